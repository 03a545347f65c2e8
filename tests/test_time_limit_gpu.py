"""-m gpu: the step counter t and the time limit T over the whole width of their 16-bit fields.

The kernels keep t in bits 16..31 of state row 0 beside agent 0's cell and held item
(csrc/oc_step_device.h: unpack / pack), env_step saturates it at 0xFFFF, build_header caps T at
65535, the branch-free `timeout` has an arm of its own for T = 0, and timestep_of() forms t / T
from a reciprocal and two FMAs.  The rest of the suite steps T <= 150: t < 128 in a positive word.
Here an episode STARTS at a chosen t -- bits 16..31 of row 0 are written after reset(), the low half
stays, and the oracle follows with ``OracleBatch.set_t`` (checked against real stepping in
test_time_limit_inputs_cpu.py, which also checks that these inputs time out, cross resets, keep
counting, set bit 15 and deliver) -- for T in {1, 2, 255, 256, 257, 32767, 32768, 49999, 65535, 0}:

  the plain fused step in five forms (generic library on four waves; level library with one lane per
    env, with two, and on one wave; structure library on two waves), the general variant (pairs and
    episode statistics) in three, the three-agent base step in two: state, done, both rewards, comm
    rows, every observation row in front of guard bytes, timestep bits and metrics against the oracle,
    every step; the timestep also against numpy's t / T, which does not rest on the oracle;
  observe() and observe_image() straight after the injection;
  a map set with T = (1, 32768, 65535) per map;
  t = 0..65535 in ONE launch of 65536 envs: observe() for 33 limits and 0, one fused step for the edges;
  OvercookedVecEnv's numpy boundary in both host_io modes and the single-env adapter at T = 65535.

T = 0: nobody times out, the timestep is t / 0.0 (inf; the pinned quiet nan at t = 0, see
test_step_prefix_gpu.py) and the state's t is min(t0 + k, 65535) -- asserted as that number, because
the oracle's plain int counts on (the counter's saturation is the one defined difference between the
two); every other field is the oracle's.

Every case prints one line "time-limit | form | T | envs that timed out | highest t in the state".
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import option_inputs as oi
import time_limit_inputs as tl
from hip_util import SENTINEL, assert_snapshots_equal, bits
from hip_util import with_margin as _with_margin

pytestmark = pytest.mark.gpu

C, RADIUS, N, STEPS = tl.C, tl.RADIUS, tl.N, tl.STEPS
FILL = 0x6B
QNAN, PINF = 0x7FF8000000000000, 0x7FF0000000000000
COUNTERS = ("env_steps", "episodes", "successes", "reward_sum", "completed_subtasks_sum", "errors")
# form -> (specialize_level, OC_LAUNCH, oc_is_specialized(), waves per 64 envs, lanes per env or None)
FORMS = {"generic-4w": (False, "split=4", 0, 4, None),
         "level-lanes1": (True, "lanes=1", 2, 4, 1),
         "level-lanes2": (True, "lanes=2", 2, 4, 2),
         "level-1w": (True, "split=1", 2, 1, None),
         "structure-2w": ("structure", "split=2", 1, 2, None)}
# general variant: form -> (specialize_level, launch hint, waves per 64 envs)
GENERAL = {"general-4w": (True, 4, 4), "general-1w": (True, 1, 1), "general-generic-1w": (False, 0, 1)}


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to("cuda:0")


def _report(form, T, timed, top):
    print("\ntime-limit | %s | %d | %d | %d" % (form, T, int(timed.sum()), int(top)))


def _expect_timestep(ts, tnum, Ts, ctx):
    """ts (device fp64 [n]) against numpy: tnum / Ts where the env has a limit (a correctly rounded
    division), t / 0.0 where it has none."""
    got = bits(ts.cpu().numpy())
    Ts = np.broadcast_to(np.asarray(Ts, np.float64), tnum.shape)
    lim = Ts != 0
    want = np.where(lim, bits(tnum.astype(np.float64) / np.where(lim, Ts, 1.0)),
                    np.where(tnum == 0, np.uint64(QNAN), np.uint64(PINF)))
    assert np.array_equal(got, want), ctx


class Tracker:
    """The counter as plain numbers beside the run: what the state must hold (saturating, 0 behind an
    auto-reset), who timed out, and the highest t a state row held."""

    def __init__(self, t0, Ts):
        self.t = np.asarray(t0).astype(np.int64)
        self.Ts = np.broadcast_to(np.asarray(Ts, np.int64), self.t.shape)
        self.timed = np.zeros(self.t.shape, bool)
        self.top = int(self.t.max())

    def step(self, done, auto_reset=True):
        done = np.asarray(done) != 0
        reached = np.minimum(self.t + 1, tl.T_MAX)
        at_limit = (self.Ts != 0) & (reached >= self.Ts)
        self.timed |= at_limit
        self.t = np.where(done & auto_reset, 0, reached)
        self.top = max(self.top, int(self.t.max()))
        return at_limit


def _snap_for(ref_snap, T, tnum, n=None):
    """The oracle's snapshot; at T = 0 with the counter as the saturating number."""
    snap = ref_snap if n is None else {k: v[:n] for k, v in ref_snap.items()}
    return dict(snap, t=tnum.astype(np.int32)) if T == 0 else snap


def _inject(env, t0, ctx):
    before = env.state.cpu().numpy()
    tl.inject_t(env, t0)
    after = env.state.cpu().numpy()
    assert np.array_equal(after[1:], before[1:]) and np.array_equal(after[0], tl.row0_with_t(before[0], t0)), ctx
    assert np.array_equal(after[0] < 0, np.asarray(t0) >= 32768), ctx
    assert np.array_equal(env.snapshot()["t"], t0), ctx


def _check_fused_step(env, out, ref, T, track, ctx):
    o, t, r, d = out
    assert np.array_equal(d.cpu().numpy(), ref["done"]), ctx
    at_limit = track.step(ref["done"])
    if T == 0:
        assert not ref["timed_out"].any(), ctx
    else:
        assert np.array_equal(at_limit, ref["timed_out"] != 0), ctx        # done by the limit exactly at the limit
    assert np.array_equal(o.cpu().numpy().astype(np.int64), ref["obs"].astype(np.int64)), ctx
    assert np.array_equal(bits(r.cpu().numpy()), bits(ref["reward"])), ctx
    assert np.array_equal(env.reward.cpu().numpy(), ref["sparse"]), ctx
    assert np.array_equal(env.comm.cpu().numpy(), ref["comm"]), ctx
    hs = env.snapshot()
    assert not hs["error"].any() and not ref["snapshot"]["error"].any(), ctx
    assert_snapshots_equal(hs, _snap_for(ref["snapshot"], T, track.t), ctx)
    if T != 0:
        assert np.array_equal(bits(t.cpu().numpy()), bits(ref["timestep"])), ctx
    _expect_timestep(t, track.t, T, ctx)


def _totals(steps, n):
    tot = dict.fromkeys(COUNTERS, 0)
    for s in steps:
        tot["env_steps"] += n
        tot["episodes"] += int(s["done"].sum())
        tot["successes"] += int(s["success"].sum())
        tot["reward_sum"] += int(s["sparse"].sum())
        tot["completed_subtasks_sum"] += int(s["completed"].sum())
        tot["errors"] += int(s["raised"].sum())
    return tot


@pytest.mark.parametrize("T", tl.LIMITS)
@pytest.mark.parametrize("form", list(FORMS))
def test_plain_fused_step_over_the_counters_range(monkeypatch, form, T):
    from gym_comm_amd.batched import BatchedOvercooked
    spec, launch, flavour, waves, lanes = FORMS[form]
    t0, steps = tl.fused_reference(T)
    acts = tl.fused_actions()
    monkeypatch.setenv("OC_LAUNCH", launch)
    env = BatchedOvercooked(tl.level(T), num_envs=N, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            auto_reset=True, specialize_level=spec)
    assert env._L.oc_is_specialized() == flavour and env.launch_waves_per_64 == waves
    if lanes is not None:
        assert env.launch_lanes() == lanes
    ctx0 = "%s T=%d" % (form, T)
    _inject(env, t0, ctx0)
    env.obs, margin = _with_margin(env.obs)
    track = Tracker(t0, T)
    acts_d = _dev(acts)
    for k in range(STEPS):
        env.obs.view(torch.uint8).fill_(FILL)
        _check_fused_step(env, env.multi_step(acts_d[k]), steps[k], T, track, "%s step %d" % (ctx0, k))
    assert bool((margin == SENTINEL).all().item()), "bytes past the last observation row were written"
    m = env.read_metrics()
    assert {c: m[c] for c in COUNTERS} == _totals(steps, N), ctx0
    assert (track.timed.sum(), track.top) == tl.table_row(t0, steps), ctx0
    _report(form, T, track.timed, track.top)


@pytest.mark.parametrize("T", tl.LIMITS)
@pytest.mark.parametrize("form", list(GENERAL))
def test_general_variant_counts_episodes_independent_of_t(monkeypatch, form, T):
    """Pairs as the action source and episode statistics on: ep_length counts by one from the
    injection on -- past the counter's saturation at T = 0 -- and ep_return adds the shaped reward."""
    from gym_comm_amd.batched import BatchedOvercooked
    spec, hint, waves = GENERAL[form]
    t0, steps = tl.fused_reference(T)
    acts = tl.fused_actions()
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    env = BatchedOvercooked(tl.level(T), num_envs=N, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            auto_reset=True, specialize_level=spec, waves_per_64=hint, episode_stats=True)
    assert env.kernel_flavour == ("spec" if spec else "generic")
    assert env.launch_waves(general=True) == waves and env.launch_lanes(general=True) == 1
    ctx0 = "%s T=%d" % (form, T)
    _inject(env, t0, ctx0)
    env.obs, margin = _with_margin(env.obs)
    track = Tracker(t0, T)
    ret, length, prev_done = np.zeros(N), np.zeros(N, np.int32), np.zeros(N, np.int32)
    longest = 0
    for k in range(STEPS):
        ctx = "%s step %d" % (ctx0, k)
        env.obs.view(torch.uint8).fill_(FILL)
        out = env.multi_step(None, ego_pairs=_dev(acts[k][0:2].T), alt_pairs=_dev(acts[k][2:4].T))
        _check_fused_step(env, out, steps[k], T, track, ctx)
        ret, length = oi.stats_step(ret, length, prev_done, steps[k]["reward"])
        assert np.array_equal(bits(env.ep_return.cpu().numpy()), bits(ret)), ctx
        assert np.array_equal(env.ep_length.cpu().numpy(), length), ctx
        prev_done = steps[k]["done"]
        longest = max(longest, int(length.max()))
    assert bool((margin == SENTINEL).all().item())
    if T == 0 or T >= 255:
        assert longest == STEPS                 # an env that never ended: the length of the window, whatever its t
    if T == 0:
        assert (track.t[t0 >= 65533] == tl.T_MAX).any() and int(length[t0 == 65535].max()) > 1
    m = env.read_metrics()
    assert {c: m[c] for c in COUNTERS} == _totals(steps, N), ctx0
    _report(form, T, track.timed, track.top)


@pytest.mark.parametrize("T", tl.LIMITS)
@pytest.mark.parametrize("form", ["step_split=1", "step_split=2"])
def test_base_step_three_agents_over_the_counters_range(monkeypatch, form, T):
    from gym_comm_amd.batched import BatchedOvercooked
    t0, steps = tl.base_reference(T)
    acts = tl.base_actions()
    monkeypatch.setenv("OC_LAUNCH", form)
    env = BatchedOvercooked(tl.level(T, tl.BASE_LEVEL, tl.BASE_AGENTS), num_envs=N, device="cuda:0", auto_reset=True,
                            specialize_level=True)
    assert env._L.oc_is_specialized() == 2 and env.A == 3
    ctx0 = "base %s T=%d" % (form, T)
    _inject(env, t0, ctx0)
    track = Tracker(t0, T)
    acts_d = _dev(acts)
    for k in range(STEPS):
        ctx = "%s step %d" % (ctx0, k)
        r, d, sh = env.step(acts_d[k])
        ref = steps[k]
        assert np.array_equal(d.cpu().numpy(), ref["done"]), ctx
        at_limit = track.step(ref["done"])
        assert np.array_equal(at_limit, ref["timed_out"] != 0), ctx
        assert np.array_equal(r.cpu().numpy(), ref["reward"]), ctx
        assert np.array_equal(bits(sh.cpu().numpy()), bits(ref["shaping"])), ctx
        hs = env.snapshot()
        assert not hs["error"].any() and not ref["snapshot"]["error"].any(), ctx
        assert_snapshots_equal(hs, _snap_for(ref["snapshot"], T, track.t), ctx)
    m = env.read_metrics()
    assert m["env_steps"] == N * STEPS and m["errors"] == 0
    assert m["episodes"] == sum(int(s["done"].sum()) for s in steps)
    assert m["reward_sum"] == sum(int(s["reward"].sum()) for s in steps)
    _report("base-" + form, T, track.timed, track.top)


@pytest.mark.parametrize("T", tl.LIMITS)
def test_observation_kernels_read_a_row_with_high_bits(monkeypatch, T):
    """observe() and observe_image() straight after the injection: the observation-only kernel and the
    image kernel unpack agent 0's cell and hand from a row 0 whose upper half is set."""
    from oracle import oracle
    from gym_comm_amd.batched import BatchedOvercooked
    oracle.build()
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    lv = tl.level(T)
    t0 = tl.start_values(T)
    ora = oracle.OracleBatch(lv.blob, N)
    ora.set_t(t0)
    want = np.zeros((2, 22 + lv.num_subtasks + 2 * C, N), np.int32)
    ts = np.zeros(N)
    for i in range(N):
        for v in range(2):
            want[v, :, i], ts[i] = ora.obs(i, v, RADIUS, False, False, C, np.zeros(2, np.int32))
    for spec in (True, "structure", False):
        env = BatchedOvercooked(lv, num_envs=N, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                                specialize_level=spec)
        ctx = "observe %s T=%d" % (spec, T)
        _inject(env, t0, ctx)
        env.obs, margin = _with_margin(env.obs)
        env.obs.view(torch.uint8).fill_(FILL)
        env.timestep.fill_(-1.0)
        o, t = env.observe()
        assert np.array_equal(o.cpu().numpy(), want), ctx
        if T != 0:
            assert np.array_equal(bits(t.cpu().numpy()), bits(ts)), ctx
        _expect_timestep(t, t0.astype(np.int64), T, ctx)
        assert bool((margin == SENTINEL).all().item()), ctx
        for radius in (0, 2, 1000):
            maps, hold = env.observe_image(radius)
            mo, ho = ora.obs_image(radius)
            assert np.array_equal(maps.cpu().numpy(), mo), ctx
            assert np.array_equal(hold.cpu().numpy().astype(np.int32), ho), ctx
        assert_snapshots_equal(env.snapshot(), ora.snapshot_all(), ctx)      # both kernels only read
    _report("observe", T, np.zeros(1, bool), int(t0.max()))


@pytest.mark.parametrize("waves", [1, 4])
def test_map_set_times_out_at_every_maps_own_limit(monkeypatch, waves):
    from gym_comm_amd.batched import BatchedOvercooked
    from test_mapset_gpu import _check_metrics, _check_step
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    t0, steps = tl.set_reference()
    acts = tl.fused_actions(tl.SET_N)
    n = tl.SET_N
    env = BatchedOvercooked.from_maps(tl.set_levels(), group_map=list(tl.SET_GROUPS), num_envs=n, device="cuda:0",
                                      num_communication=C, fow_radius=RADIUS, auto_reset=True, waves_per_64=waves)
    assert env._L.oc_is_specialized() == 1 and env.launch_waves() == waves
    Ts = np.asarray(tl.SET_T)[tl.set_env_map()]
    ctx0 = "map set waves=%d" % waves
    _inject(env, t0, ctx0)
    track = Tracker(t0, Ts)
    acts_d = _dev(acts)
    for k in range(STEPS):
        ctx = "%s step %d" % (ctx0, k)
        out = env.multi_step(acts_d[k])
        _check_step(env, out, steps[k], ctx)
        at_limit = track.step(steps[k]["done"])
        done = out[3].cpu().numpy() != 0
        assert np.array_equal(done & (steps[k]["success"] == 0), at_limit), ctx     # at its own map's T
        assert np.array_equal(env.snapshot()["t"], track.t), ctx
        _expect_timestep(out[1], track.t, Ts, ctx)
    _check_metrics(env, steps, list(tl.SET_MAPS), ctx0)
    per_map = env.read_metrics()["per_map"]
    assert per_map[0]["episodes"] == 64 * STEPS                # T = 1: every env, every step
    for m, T in enumerate(tl.SET_T):
        sel = tl.set_env_map() == m
        _report("mapset-%dw-map%d" % (waves, m), T, track.timed[sel], max(int(t0[sel].max()), 0))


# ---- the quotient over the whole field -----------------------------------------------------------
SWEEP_N = 1 << 16


@pytest.mark.parametrize("T", tl.sweep_limits() + [0])
def test_observe_divides_every_t_by_T(monkeypatch, T):
    """Env i holds t = i, i = 0..65535: the whole range of the field in one launch of the
    observation-only kernel, against numpy's correctly rounded division."""
    from gym_comm_amd.batched import BatchedOvercooked
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    env = BatchedOvercooked(tl.level(T), num_envs=SWEEP_N, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            specialize_level=True, track_metrics=False)
    t = np.arange(SWEEP_N)
    tl.inject_t(env, t)
    env.timestep.fill_(-1.0)
    _, ts = env.observe()
    _expect_timestep(ts, t, T, "observe sweep T=%d" % T)
    assert np.array_equal(env.snapshot()["t"], t)


SWEEP_FORMS = {"generic-4w": (False, "split=4", 4), "generic-1w": (False, "split=1", 1),
               "level-4w": (True, "split=4", 4), "level-1w": (True, "split=1", 1)}


@pytest.mark.parametrize("T", tl.LIMITS)
@pytest.mark.parametrize("form", list(SWEEP_FORMS))
def test_one_fused_step_counts_and_divides_every_t(monkeypatch, form, T):
    """Env i holds t = i - 1 (env 0: 65535, which a step leaves at 65535); one fused step without
    auto-reset: every other env's counter is i, done is set from T on and nowhere below (nobody
    delivers on the first step), and the timestep is the new counter over T -- compared for EVERY
    env, the finished ones included (their rows are the final state's)."""
    from gym_comm_amd.batched import BatchedOvercooked
    spec, launch, waves = SWEEP_FORMS[form]
    monkeypatch.setenv("OC_LAUNCH", launch)
    env = BatchedOvercooked(tl.level(T), num_envs=SWEEP_N, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            auto_reset=False, specialize_level=spec)
    assert env.launch_waves_per_64 == waves and env._L.oc_is_specialized() == (2 if spec else 0)
    t = (np.arange(SWEEP_N) - 1) % SWEEP_N
    tl.inject_t(env, t)
    track = Tracker(t, T)
    acts = torch.zeros((4, SWEEP_N), dtype=torch.int32, device="cuda:0")
    _, ts, _, d = env.multi_step(acts)
    ctx = "fused sweep %s T=%d" % (form, T)
    want_done = (T != 0) & (np.minimum(track.t + 1, tl.T_MAX) >= T)
    assert np.array_equal(d.cpu().numpy() != 0, want_done), ctx
    track.step(want_done, auto_reset=False)
    assert track.t[0] == track.t[-1] == tl.T_MAX and track.t[1] == 1
    assert np.array_equal(env.snapshot()["t"], track.t), ctx
    _expect_timestep(ts, track.t, T, ctx)
    m = env.read_metrics()
    assert m["env_steps"] == SWEEP_N and m["episodes"] == int(want_done.sum()) and m["errors"] == 0
    _report("sweep-" + form, T, want_done, track.top)


# ---- the numpy boundary and the single-env adapter -------------------------------------------------
def _arglist(T):
    return SimpleNamespace(level=tl.LEVEL, num_agents=2, max_num_timesteps=T, ego_config={}, partner_config={},
                           num_communication=C, communication_on=True, ego_led=False, fow_radius=RADIUS)


@pytest.mark.parametrize("host_io", ["copy", "mapped"])
def test_vec_env_reports_the_timestep_and_the_limit_at_65535(monkeypatch, host_io):
    from gym_comm_amd.vec_env import OvercookedVecEnv
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    T, n = 65535, 130
    venv = OvercookedVecEnv(_arglist(T), n, seed=9, host_io=host_io)
    venv.reset()
    t0 = tl.start_values(T, n)
    _inject(venv._b, t0, "vec env")
    track = Tracker(t0, T)
    rng = np.random.default_rng(tl.SEED + 3)
    ended = 0
    for k in range(5):
        actions = np.stack([rng.integers(0, 4, n), rng.integers(0, C, n)], axis=1)
        obs, rew, dones, infos = venv.step(actions)
        ctx = "vec env %s step %d" % (host_io, k)
        at_limit = track.step(track.t + 1 >= T)            # (nobody delivers within five steps of a reset)
        assert dones.dtype == bool and np.array_equal(dones, at_limit), ctx
        ts = obs["timestep"]
        assert ts.dtype == np.float32 and ts.shape == (n, 1), ctx
        want = (track.t.astype(np.float64) / T).astype(np.float32)
        assert np.array_equal(ts[:, 0].view(np.uint32), want.view(np.uint32)), ctx
        lengths = venv.episode_lengths.cpu().numpy()
        for i in np.nonzero(dones)[0]:
            assert infos[i]["episode"]["l"] == int(lengths[i]) == k + 1, ctx
            ended += 1
        for i in np.nonzero(~dones)[0][:3]:
            assert "episode" not in infos[i], ctx
        probe = [0, 2, 28, 29, 129]
        assert venv.get_attr("t", probe) == [int(track.t[i]) for i in probe], ctx
    assert ended == int(track.timed.sum()) >= 20 and track.top == T - 1      # t0 = T - 1 .. T - 5, five envs each
    venv.close()
    _report("vec-env-" + host_io, T, track.timed, track.top)


@pytest.mark.parametrize("t0,steps", [(40000, 3), (65532, 3)])
def test_single_env_adapter_reports_the_injected_t_plus_the_steps(monkeypatch, t0, steps):
    from gym_comm_amd.envs import OvercookedEnvironment
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    T = 65535
    env = OvercookedEnvironment(_arglist(T), device="cuda:0")
    _inject(env._b, np.array([t0]), "adapter")
    env.mark_dirty()
    assert env.t == t0
    stay = {name: (0, 0) for name in env.get_agent_names()}
    for k in range(steps):
        r, d, info = env.step(stay)
        assert info["t"] == env.t == t0 + k + 1 and r == 0
        assert d == (t0 + k + 1 >= T) and info["done"] == d
        assert env.termination_info == ("Terminating because passed %d timesteps" % T if d else "")
    assert d == (t0 + steps >= T)
