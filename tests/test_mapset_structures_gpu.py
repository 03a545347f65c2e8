"""-m gpu: map sets (BatchedOvercooked.from_maps) on the structures and options test_mapset_gpu.py never
ran, against one CPU oracle per map (its SetOracle).  Inputs: tests/mapset_inputs.py; that they reach what
each case is about is checked without a GPU in test_mapset_structures_cpu.py.  Every comparison is on bits.

  the shipped random-* Salad family -- seven maps of 9 to 29 Counters, nine groups, a 37-env last group --
    with the in-kernel draw: the drawn cells are read back after the reset and after every auto-reset,
    must be distinct Counters of the env's OWN map and go to that map's oracle; state, rows, timestep,
    rewards, done and comm after every step, the counters per map at the end; every Counter of every map
    is drawn (the miss probability is bounded in the test); get_state / set_state carry the placement stream;
  four of those maps on host placements: the constructor's reset starts each env on its own map's nominal
    cells; then per-env cells refilled before every step;
  the cramped map (the reference raises on it) between two clean ones: error bits env by env, errors per map;
  two maps that repeat a type (the DUP kernels and the two extra state words);
  three Salad maps with a time limit each; the tl maps in a caller's subtask order; OvercookedVecEnv on
    three random maps, and its numpy step through host-mapped buffers against the copying twin."""
import types

import numpy as np
import pytest
import torch

import mapset_inputs as mi
import option_inputs as oi
from hip_util import assert_snapshots_equal, bits
from test_mapset_gpu import C, RADIUS, SetOracle, _check_metrics, _check_step, _dev

pytestmark = pytest.mark.gpu

CASE_IDS = lambda v: str(v).replace("torch.", "")  # noqa: E731


def _make(case, waves, dtype=torch.int32, stats=False, levels=None, **kw):
    from gym_comm_amd.batched import BatchedOvercooked
    _, _, gm, n, _, _ = mi.CASES[case]
    env = BatchedOvercooked.from_maps(levels or mi.case_levels(case), group_map=list(gm), num_envs=n, device="cuda:0",
                                      num_communication=C, fow_radius=RADIUS, auto_reset=True, obs_dtype=dtype,
                                      episode_stats=stats, waves_per_64=waves, **kw)
    assert env.kernel_flavour == "spec" and env._L.oc_is_specialized() == 1
    assert env.launch_waves(general=stats) == waves and env.launch_lanes() == 1       # the launch taken
    return env


def _state_cells(env):
    """Packed item cells (x | y<<4) [M][n] read back from the device state."""
    return (env.state[env.A:env.A + env.M].cpu().numpy() & 255).astype(np.int32)


class _Partner:
    """XO = 1: the in-kernel partner's stream and what it played, and the episode statistics, against
    their numpy restatements (option_inputs.py) at every step."""

    def __init__(self, case):
        self.acts, self.words = mi.actions(case)
        n = self.acts.shape[2]
        self.stream = _dev(self.words[0])
        self.played = torch.zeros((2, n), dtype=torch.int32, device="cuda:0")
        self.ret, self.length, self.prev_done = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)

    def step(self, env, k):
        return env.multi_step(None, ego_pairs=_dev(self.acts[k][0:2].T), alt_rng=self.stream, alt_played=self.played)

    def check(self, env, k, ref, ctx):
        assert np.array_equal(self.stream.cpu().numpy(), self.words[k + 1]), ctx
        assert np.array_equal(self.played.cpu().numpy(), self.acts[k][2:4]), ctx
        self.ret, self.length = oi.stats_step(self.ret, self.length, self.prev_done, ref["reward"])
        assert np.array_equal(bits(env.ep_return.cpu().numpy()), bits(self.ret)), ctx
        assert np.array_equal(env.ep_length.cpu().numpy(), self.length), ctx
        self.prev_done = ref["done"]

    def start_over(self, env, mask):
        """After a reset by hand the caller starts the envs' statistics over (as reset_tensors does for all)."""
        hit = _dev(mask).bool()
        env.ep_return[hit], env.ep_length[hit] = 0.0, 0
        self.ret, self.length = np.where(mask != 0, 0.0, self.ret), np.where(mask != 0, 0, self.length).astype(np.int32)


def _check_state(env, ref, ctx):
    """The full state and the error bits, env by env (a flagged env too: the defined result)."""
    snap = env.snapshot()
    assert np.array_equal(snap["error"], ref["snapshot"]["error"]), ctx
    assert_snapshots_equal(snap, ref["snapshot"], ctx)


def _run_known(case, env, xo, dtype=torch.int32, refill=False):
    """A case whose placements are known ahead, against mapset_inputs.reference: every step's full state
    and error bits, rows, timestep, rewards, done and comm; XO = 1: the partner and the statistics; the
    counters in total and per map.  ``refill``: the placement tensor takes host_cells(case, k) before
    step k, which is where the oracle re-places the envs that finish at step k."""
    names, Ts, gm, n, steps, _ = mi.CASES[case]
    acts, _ = mi.actions(case)
    refs = mi.reference(case)
    ctx0 = "%s waves=%d xo=%d %s" % (case, env.launch_waves(general=bool(xo)), xo, str(dtype)[6:])
    _check_state(env, refs[0], ctx0 + " after reset")
    partner = _Partner(case) if xo else None
    episodes = np.zeros(n, np.int64)
    for k in range(steps):
        ctx = "%s step %d" % (ctx0, k)
        if refill:
            env.set_placement(_dev(mi.host_cells(case, k)))
        out = partner.step(env, k) if xo else env.multi_step(_dev(acts[k]))
        assert out[0].dtype == dtype
        ref = refs[k + 1]
        _check_step(env, out, ref, ctx, snapshot=False)
        _check_state(env, ref, ctx)
        if xo:
            partner.check(env, k, ref, ctx)
        episodes += ref["done"] != 0
        mask = mi.stagger_mask(case, k)
        if mask is not None:            # a reset by hand that cuts through every group
            env.reset(_dev(mask))
            if xo:
                partner.start_over(env, mask)
    assert (episodes >= steps // np.asarray(Ts)[mi.env_map(case)]).all(), ctx0
    _check_metrics(env, refs[1:], [lv.name for lv in mi.case_levels(case)], ctx0)
    return refs


# ---- 1. the random Salad family, in-kernel draw --------------------------------------------------
class _Draws:
    """The cells the library drew, read back from the state: every one a Counter of the env's own map,
    an env's three distinct; per map a histogram of the Counters drawn by the step kernel's auto-resets and
    one of those drawn by oc_mapset_reset (two kernels, two look-ups of the group's record)."""

    def __init__(self, case):
        self.lvs, self.em = mi.case_levels(case), mi.env_map(case)
        self.cc = [np.sort(mi.counter_cells(lv)) for lv in self.lvs]
        self.hist = {by: [np.zeros(len(cc), np.int64) for cc in self.cc] for by in ("step", "reset")}
        self.resets = np.zeros(len(self.em), np.int64)

    def miss_bound(self, resets_per_env):
        """An env-reset draws 3 of a map's c Counters without replacement, so it misses a given one with
        probability (c - 3) / c; r independent env-resets miss at least one of the c Counters with
        probability at most c ((c - 3) / c)^r (union bound)."""
        return max(len(cc) * ((len(cc) - 3.0) / len(cc)) ** (int((self.em == m).sum()) * resets_per_env)
                   for m, cc in enumerate(self.cc))

    def assert_every_counter_drawn(self, by, ctx):
        for m, lv in enumerate(self.lvs):
            h = self.hist[by][m]
            assert (h > 0).all(), "%s: Counters of %s never drawn by the %s kernel: %s" % (
                ctx, lv.name, by, [int(c) for c in self.cc[m][h == 0]])

    def read(self, env, mask, ctx, by="step"):
        cells = _state_cells(env)
        for m, cc in enumerate(self.cc):
            sub = cells[:, (self.em == m) & mask]
            assert np.isin(sub, cc).all(), "%s: a cell that is no Counter of %s" % (ctx, self.lvs[m].name)
            assert all(len(set(sub[:, j].tolist())) == env.M for j in range(sub.shape[1])), ctx
            self.hist[by][m] += np.bincount(np.searchsorted(cc, sub.reshape(-1)), minlength=len(cc))
        self.resets += mask
        return cells


def _run_drawn(case, env, ora, xo, steps, dtype, ctx0, acts, partner=None, step=None):
    """placement_mode="rng" against SetOracle: the oracle steps with auto_reset off; the envs that
    finished are re-placed on the cells read back from the library's state (SetOracle.replace_finished),
    so the rows and the timestep of a finished env are compared with the re-placed episode's first
    observation, everything else with the step's own results."""
    draws = _Draws(case)
    n = len(draws.em)
    ora.set_placement(draws.read(env, np.ones(n, bool), ctx0, by="reset"))
    ora.reset()
    assert_snapshots_equal(env.snapshot(), ora.snapshot(), ctx0 + " after reset")
    refs = []
    for k in range(steps):
        ctx = "%s step %d" % (ctx0, k)
        out = step(k) if step else (partner.step(env, k) if xo else env.multi_step(_dev(acts[k])))
        a = acts[k] if step is None else np.concatenate([acts[k][0:2], step.played()])
        ref = ora.multi_step(a, auto_reset=False)
        assert np.array_equal(out[3].cpu().numpy(), ref["done"]), ctx
        ora.replace_finished(ref, draws.read(env, ref["done"] != 0, ctx))
        assert out[0].dtype == dtype
        _check_step(env if step is None else step.batch, out, ref, ctx)        # (the state; no flag anywhere)
        assert int(ref["raised"].sum()) == 0, ctx
        if partner:
            partner.check(env, k, ref, ctx)
        refs.append(ref)
    return draws, refs


FAMILY_CASES = [(1, 0, torch.int32), (4, 0, torch.int32), (1, 1, torch.int32), (4, 1, torch.int32),
                (4, 0, torch.int8), (4, 1, torch.float32)]


@pytest.mark.parametrize("waves,xo,dtype", FAMILY_CASES, ids=CASE_IDS)
def test_random_salad_family_in_kernel_draw(monkeypatch, waves, xo, dtype):
    """Seven maps whose Counter counts, table sizes and table addresses all differ: a draw made with
    another map's `ncounters` or Counter block lands on a cell that is no Counter of the env's map, or
    never reaches that map's high Counters.  XO = 1 runs two PCG32 streams per env -- the placement's and
    the partner's -- and both are followed."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "family"
    names, Ts, gm, n, steps, _ = mi.CASES[case]
    env = _make(case, waves, dtype, stats=bool(xo), placement_mode="rng", seed=11)
    assert env.rng is not None and env.placement is None
    ctx0 = "family waves=%d xo=%d %s" % (waves, xo, str(dtype)[6:])
    acts, _ = mi.actions(case)
    partner = _Partner(case) if xo else None
    probe = _Draws(case)
    # before the coverage below is relied on: the step kernel re-places every env at least steps // T = 4
    # times (the constructor's reset is another kernel's draw and counted apart), and with them the chance
    # that some Counter of a map is never drawn by it is below 1e-9 for every map
    assert probe.miss_bound(steps // Ts[0]) < 1e-9 and probe.miss_bound(1 + steps // Ts[0]) < 1e-9
    draws, refs = _run_drawn(case, env, SetOracle(mi.case_levels(case), gm, n), xo, steps, dtype, ctx0, acts, partner)
    assert draws.resets.min() >= 1 + steps // Ts[0], ctx0
    draws.assert_every_counter_drawn("step", ctx0)
    _check_metrics(env, refs, list(names), ctx0)


def test_random_salad_family_reset_draws_reach_every_counter(monkeypatch):
    """oc_mapset_reset's own draw: the constructor's reset and five more, each read back, checked (distinct
    Counters of the env's own map) and compared with the oracles reset on those cells.  Six resets per env
    miss some Counter of a map with probability below 1e-9 (asserted first)."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "family"
    _, _, gm, n, _, _ = mi.CASES[case]
    env = _make(case, 4, placement_mode="rng", seed=13)
    draws, ora = _Draws(case), SetOracle(mi.case_levels(case), gm, n)
    assert draws.miss_bound(6) < 1e-9
    for k in range(6):
        if k:
            env.reset()
        ora.set_placement(draws.read(env, np.ones(n, bool), "reset %d" % k, by="reset"))
        ora.reset()
        assert_snapshots_equal(env.snapshot(), ora.snapshot(), "reset %d" % k)
    draws.assert_every_counter_drawn("reset", "six resets")


def test_random_salad_family_state_round_trip_carries_the_placement_stream(monkeypatch):
    """get_state in the middle of an episode, 30 steps across an auto-reset of every env (T = 25), back,
    the same 30 steps: every fetched array and the placement stream byte for byte."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "family"
    acts, _ = mi.actions(case)
    env = _make(case, 4, placement_mode="rng", seed=11)
    for k in range(10):
        env.multi_step(_dev(acts[k]))
    saved = env.get_state()
    rng0 = env.rng.clone()
    runs = []
    for _ in range(2):
        rec, resets = [], np.zeros(env.n, np.int64)
        for k in range(10, 40):
            env.multi_step(_dev(acts[k]))
            rec.append((env.fetch(), env.rng.cpu().numpy().copy()))
            resets += rec[-1][0]["done"] != 0
        assert resets.min() >= 1
        runs.append((rec, env.metrics.clone()))
        assert not torch.equal(env.rng, rng0)            # (the stream moved: every env drew again)
        env.set_state(saved)
        assert torch.equal(env.rng, rng0)
    for k, ((a, ra), (b, rb)) in enumerate(zip(runs[0][0], runs[1][0])):
        assert np.array_equal(ra, rb), "rng step %d" % (10 + k)
        for name in a:
            assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), "%s step %d" % (name, 10 + k)
    assert torch.equal(runs[0][1], runs[1][1])


# ---- 2. host placement ---------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
def test_host_placement_per_map(monkeypatch, waves):
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "host"
    _, _, gm, n, _, _ = mi.CASES[case]
    env = _make(case, waves, placement_mode="host")
    # the constructor's own reset, before any set_placement: each env on ITS map's nominal cells
    nominal = mi.nominal_cells(case)
    ora = SetOracle(mi.case_levels(case), gm, n)
    ora.set_placement(nominal)
    ora.reset()
    assert np.array_equal(env.placement.cpu().numpy(), nominal)
    assert np.array_equal(_state_cells(env), nominal)
    assert_snapshots_equal(env.snapshot(), ora.snapshot(), "host waves=%d after the constructor" % waves)
    env.set_placement(_dev(mi.host_cells(case, -1)))
    env.reset()
    _run_known(case, env, 0, refill=True)


# ---- 3. the cramped map --------------------------------------------------------------------------
def test_cramped_map_in_a_set_flags_and_counts_errors_per_map(monkeypatch):
    """random-open-divider_salad_small_cramped starts agent 0 in the (0, 0) corner, where the reference
    raises; it sits in the middle group between two clean maps.  The flags of every env after every step,
    every defined result, and `errors` per map: the oracle's count on the cramped map, 0 on the others --
    the one counter a slot-to-map mix-up cannot hide in."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "cramped"
    names = mi.CASES[case][0]
    env = _make(case, 4, placement_mode="host")
    refs = _run_known(case, env, 0)
    want = [sum(int(r["raised"][mi.env_map(case) == m].sum()) for r in refs[1:]) for m in range(3)]
    got = env.read_metrics()
    assert names[1] == mi.CRAMPED and want[1] > 100 and want[0] == want[2] == 0
    assert [p["errors"] for p in got["per_map"]] == want and got["errors"] == want[1]


# ---- 4. maps that repeat a type ------------------------------------------------------------------
@pytest.mark.parametrize("waves,xo", [(1, 0), (4, 0), (1, 1), (4, 1)])
def test_set_of_maps_that_repeat_a_type(monkeypatch, waves, xo):
    """The DUP = true instantiations of k_mapset_step / _obs / _reset: custom-two_tomatoes and a variant
    with another interior.  The state carries two more words (the key-creation sequence): `order` and
    the 2-bit goal counts of the snapshot come from them."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    env = _make("dup", waves, stats=bool(xo))
    assert env._dup and env.W_state == env.A + env.M + 4 and tuple(env.state.shape) == (env.W_state, env.n)
    refs = _run_known("dup", env, xo)
    assert any((r["snapshot"]["goal_count"] >= 2).any() for r in refs)


# ---- 5. per-map T, tl, the vec env ----------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
def test_each_map_keeps_its_own_time_limit(monkeypatch, waves):
    """MapRecord.R is per map: T = 12, 25 and 40.  Each env times out at its own map's T, its timestep
    row is t (1 / T) of that T on bits, and ep_length at a finished env is its T or the delivery step."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "per-map-T"
    _, Ts, _, n, steps, _ = mi.CASES[case]
    env = _make(case, waves, stats=True)
    assert [lv.max_num_timesteps for lv in env.levels] == list(Ts)
    refs = _run_known(case, env, 1)
    t_env = np.asarray(Ts)[mi.env_map(case)]
    # (from the reference the kernel was just shown equal to) the finished envs' lengths, restated
    length, prev = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for k in range(steps):
        r = refs[k + 1]
        _, length = oi.stats_step(np.zeros(n), length, prev, r["reward"])
        prev = r["done"]
        fin = r["done"] != 0
        assert ((length[fin] == t_env[fin]) | (r["success"][fin] != 0)).all(), k
        assert (length[fin] <= t_env[fin]).all(), k
        if mi.stagger_mask(case, k) is not None:        # (started over with the reset by hand)
            length = np.where(mi.stagger_mask(case, k) != 0, 0, length).astype(np.int32)
    assert np.array_equal(env.ep_length.cpu().numpy(), length)


def test_tl_maps_in_a_callers_subtask_order(monkeypatch):
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "tl"
    names, Ts, gm, n, steps, _ = mi.CASES[case]
    # by name: from_maps compiles the maps itself, in the caller's order
    env = _make(case, 4, torch.float32, levels=list(names), subtask_order=mi.TL_ORDER, max_num_timesteps=Ts[0])
    assert env.S == 6 and env.F == 22 + 6 + 2 * C
    for got, want in zip(env.levels, mi.case_levels(case)):
        assert np.array_equal(got.blob, want.blob)
    refs = _run_known(case, env, 0, torch.float32)
    lo, hi = env._layout["completed_subtasks"]
    assert np.array_equal(env.completed_subtasks().cpu().numpy(), refs[-1]["snapshot"]["completed"].T)
    assert np.array_equal(env.obs[0, lo:hi].cpu().numpy().astype(np.int32), refs[-1]["obs"][0, lo:hi])
    assert sum(int(r["snapshot"]["completed"].sum()) for r in refs) > 0


def _arglist(level):
    return types.SimpleNamespace(level=level, num_agents=2, max_num_timesteps=25, max_num_subtasks=14,
                                 ego_config={}, partner_config={}, num_communication=C, communication_on=True,
                                 ego_led=False, fow_radius=RADIUS, play=False)


class _VecStep:
    def __init__(self, venv, acts):
        self.venv, self.acts, self.batch = venv, acts, venv._b

    def __call__(self, k):
        self.obs, rew, done = self.venv.step_tensors(_dev(self.acts[k][0:2].T))
        return self.batch.obs, self.batch.timestep, rew, done

    def played(self):
        return self.venv._act[2:4].cpu().numpy()         # what the in-kernel partner drew


def test_vec_env_on_three_random_maps_and_the_mapped_numpy_step(monkeypatch):
    from gym_comm_amd.vec_env import OvercookedVecEnv
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    case = "vec-env"
    names, _, gm, n, steps, _ = mi.CASES[case]
    acts, _ = mi.actions(case)
    venvs = [OvercookedVecEnv(_arglist(names[0]), n, device="cuda:0", levels=list(names), seed=5, host_io=io)
             for io in ("mapped", "copy")]
    venv, twin = venvs
    assert [venv._b.map_of(i) for i in (0, 64, n - 1)] == list(names) and venv._b.rng is not None
    for v in venvs:
        v.reset_tensors()
    step = _VecStep(venv, acts)
    _run_drawn(case, venv._b, SetOracle(mi.case_levels(case), gm, n), 1, steps, torch.int32, "vec-env", acts,
               step=step)
    for k in range(steps):
        twin.step_tensors(_dev(acts[k][0:2].T))
    assert torch.equal(venv._b.state, twin._b.state) and torch.equal(venv._b.rng, twin._b.rng)
    # one step through the numpy API: host-mapped buffers against staged copies
    a = np.ascontiguousarray(acts[steps - 1][0:2].T)
    (oa, ra, da, ia), (ob, rb, db, ib) = venv.step(a), twin.step(a)
    assert sorted(oa) == sorted(ob) and len(oa) >= 10
    for key in oa:
        assert oa[key].dtype == ob[key].dtype and np.array_equal(oa[key], ob[key]), key
    assert np.array_equal(bits(ra), bits(rb)) and np.array_equal(da, db) and ia == ib
    assert torch.equal(venv._b.state, twin._b.state) and torch.equal(venv._b.rng, twin._b.rng)
    for v in venvs:
        v.close()
