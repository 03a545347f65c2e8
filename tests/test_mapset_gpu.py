"""-m gpu: map sets (BatchedOvercooked.from_maps, include/oc_hip.h: oc_mapset_*) -- envs on different
maps of one structure stepped by ONE launch -- against one CPU oracle per map, run on that map's envs.
Every comparison is on bits.

  three shipped maps, n = 229 with a 37-env last group, T = 25 and 120 steps (every env auto-resets at
    least four times): state, comm, both viewers' rows, timestep, shaped and sparse reward and done after
    every step, per-map and total metrics at the end; one wave and four waves per 64 envs (forced by the
    launch hint); XO = 0 (the four action rows) and XO = 1 (int32 pairs + the in-kernel partner + episode
    statistics: the partner's actions of EVERY run are that draw, restated in numpy, so one oracle run
    serves them all); int8 and float32 rows once each at four waves;
  two maps of different sizes: a shipped 7x7 tomato map and a 6x5 map written here (the same recipe and
    items, closed border, the Delivery tile elsewhere);
  a set whose groups all name map 0 against the single-level batch on the same structure library;
  reset(mask) with a mask that cuts through groups + observe(); get_state / set_state mid-episode;
  OvercookedVecEnv(levels=[...]): step_tensors, a captured ClosedLoop against the eager one, base_env;
  oc_mapset_create's refusals in the level library and the generic library (return codes only)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import option_inputs as oi
from hip_util import assert_snapshots_equal, bits, momentum_actions

pytestmark = pytest.mark.gpu

C, RADIUS, T, SEED = 3, 2, 25, 23
TOMATO = ["open-divider_tomato", "partial-divider_tomato", "full-divider_tomato"]
COUNTERS = ("env_steps", "episodes", "successes", "reward_sum", "completed_subtasks_sum", "errors")
# 6 x 5, the tomato levels' structure: Tomato, Lettuce, two Plates in that scan order, SimpleTomato, a
# closed border; Delivery on the right-hand wall
SMALL_MAP = "-t-l--\n/    -\n-    *\np    p\n------\n\nSimpleTomato\n\n1 1\n3 2\n"


def _levels(names):
    from gym_comm_amd import compiler, levels
    out = []
    for name in names:
        spec = levels.parse_level_text("small-tomato", SMALL_MAP) if name == "small-tomato" else name
        out.append(compiler.compile_level(spec, 2, T))
    return out


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(n, steps):
    """Seeded actions [steps][4][n] -- the partner's are the in-kernel partner's own draw -- and that
    partner's stream words [steps + 1][n] (int32 bit patterns)."""
    from gym_comm_amd.batched import pcg32_seed_states
    rng = np.random.default_rng(SEED)
    mv = momentum_actions(rng, steps, 1, n, keep=0.6, nact=4)[:, 0]
    cm = rng.integers(0, C, (steps, n))
    s = pcg32_seed_states(SEED, (n,)).numpy().astype(np.int64).astype(np.uint64)
    words, pmv, pcm = [s], [], []
    for _ in range(steps):
        s, m, c = oi.partner_draw(s, C)
        words.append(s), pmv.append(m), pcm.append(c)
    acts = np.stack([mv, cm, np.stack(pmv), np.stack(pcm)], axis=1).astype(np.int32)
    words = np.stack(words).astype(np.uint32).view(np.int32)
    acts.setflags(write=False), words.setflags(write=False)
    return acts, words


class SetOracle:
    """One OracleBatch per map over that map's envs; inputs and outputs in the batch's env order."""

    def __init__(self, lvs, group_map, n):
        from oracle import oracle
        self.n, self.lvs = n, lvs
        env_map = np.asarray(group_map)[np.arange(n) // 64]
        self.idx = [np.nonzero(env_map == m)[0] for m in range(len(lvs))]
        self.ora = [oracle.OracleBatch(lv.blob, len(ix)) if len(ix) else None for lv, ix in zip(lvs, self.idx)]
        self.comm = [np.zeros((2, len(ix)), np.int32) for ix in self.idx]
        self.S = lvs[0].num_subtasks

    def _each(self):
        return [(m, o, ix) for m, (o, ix) in enumerate(zip(self.ora, self.idx)) if o is not None]

    def reset(self, mask=None):
        for m, o, ix in self._each():
            o.reset(None if mask is None else np.ascontiguousarray(mask[ix]))

    def snapshot(self):
        out = None
        for m, o, ix in self._each():
            s = o.snapshot_all()
            if out is None:
                out = {k: np.zeros((self.n,) + v.shape[1:], v.dtype) for k, v in s.items()}
            for k, v in s.items():
                out[k][ix] = v
        return out

    def set_placement(self, cells):
        """[M][n] packed start cells in the batch's env order; every map's oracle gets its own envs' columns."""
        for m, o, ix in self._each():
            o.set_placement(np.ascontiguousarray(np.asarray(cells)[:, ix]))

    def multi_step(self, acts, auto_reset=True):
        n, F = self.n, 22 + self.S + 2 * C
        r = {"obs": np.zeros((2, F, n), np.int32), "timestep": np.zeros(n), "reward": np.zeros(n),
             "done": np.zeros(n, np.int32), "comm": np.zeros((2, n), np.int32), "sparse": np.zeros(n, np.int32),
             "raised": np.zeros(n, np.int32), "success": np.zeros(n, np.int32), "per_map": []}
        for m, o, ix in self._each():
            obs, ts, rew, done = o.multi_step(np.ascontiguousarray(acts[:, ix]), self.comm[m], RADIUS, 0, C,
                                              auto_reset=auto_reset)
            last = o.last_step()
            r["obs"][:, :, ix], r["timestep"][ix], r["reward"][ix], r["done"][ix] = obs, ts, rew, done
            r["comm"][:, ix], r["sparse"][ix] = self.comm[m], last["sparse"]
            r["raised"][ix], r["success"][ix] = last["raised"], last["success"]
            r["per_map"].append((m, {"env_steps": len(ix), "episodes": int(done.sum()),
                                     "successes": int(last["success"].sum()), "reward_sum": int(last["sparse"].sum()),
                                     "completed_subtasks_sum": int(last["completed"].sum()),
                                     "errors": int(last["raised"].sum())}))
        r["snapshot"] = self.snapshot()
        return r

    def replace_finished(self, r, cells):
        """After ``multi_step(acts, auto_reset=False)``: the envs that finished start their next episode on
        ``cells`` ([M][n]: a placement nobody can know ahead, such as the library's own draw) -- a masked
        reset -- and their rows and timestep in ``r`` become that episode's first observation."""
        self.set_placement(cells)
        self.reset(r["done"])
        for m, o, ix in self._each():
            for j, i in enumerate(ix):
                if r["done"][i]:
                    for v in range(2):
                        r["obs"][v, :, i], r["timestep"][i] = o.obs(j, v, RADIUS, False, False, C,
                                                                    [int(self.comm[m][0, j]), int(self.comm[m][1, j])])
        r["snapshot"] = self.snapshot()
        return r


@functools.lru_cache(maxsize=None)
def _reference(names, group_map, n, steps):
    """The oracles' results of every step, computed once and shared (read-only)."""
    lvs = _levels(names)
    acts, _ = _inputs(n, steps)
    ora = SetOracle(lvs, group_map, n)
    ora.reset()
    out = [ora.multi_step(acts[k]) for k in range(steps)]
    for r in out:
        for v in list(r.values()) + list(r["snapshot"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def _make(names, group_map, n, waves, dtype=torch.int32, stats=False):
    from gym_comm_amd.batched import BatchedOvercooked
    env = BatchedOvercooked.from_maps(_levels(names), group_map=list(group_map), num_envs=n, device="cuda:0",
                                      num_communication=C, fow_radius=RADIUS, auto_reset=True, obs_dtype=dtype,
                                      episode_stats=stats, waves_per_64=waves)
    assert env.kernel_flavour == "spec" and env._L.oc_is_specialized() == 1
    assert env.launch_waves(general=stats) == waves and env.launch_lanes() == 1       # the launch taken
    return env


def _check_step(env, out, ref, ctx, snapshot=True):
    o, t, r, d = out
    assert np.array_equal(d.cpu().numpy(), ref["done"]), ctx
    assert np.array_equal(o.cpu().numpy().astype(np.int64), ref["obs"].astype(np.int64)), ctx
    assert np.array_equal(bits(t.cpu().numpy()), bits(ref["timestep"])), ctx
    assert np.array_equal(bits(r.cpu().numpy()), bits(ref["reward"])), ctx
    assert np.array_equal(env.comm.cpu().numpy(), ref["comm"]), ctx
    assert np.array_equal(env.reward.cpu().numpy(), ref["sparse"]), ctx
    if snapshot:
        assert_snapshots_equal(env.snapshot(), ref["snapshot"], ctx)
        assert int(np.count_nonzero(env.snapshot()["error"])) == 0, ctx


def _check_metrics(env, refs, names, ctx):
    K = len(names)
    per_map = [dict.fromkeys(COUNTERS, 0) for _ in range(K)]
    for r in refs:
        for m, counts in r["per_map"]:
            for c in COUNTERS:
                per_map[m][c] += counts[c]
    got = env.read_metrics()
    assert {c: got[c] for c in COUNTERS} == {c: sum(p[c] for p in per_map) for c in COUNTERS}, ctx
    assert len(got["per_map"]) == K
    for m in range(K):
        assert {c: got["per_map"][m][c] for c in COUNTERS} == per_map[m], "%s map %d" % (ctx, m)
        assert got["per_map"][m]["level"] == names[m]


def _run(names, group_map, n, steps, waves, xo, dtype=torch.int32):
    acts, words = _inputs(n, steps)
    refs = _reference(tuple(names), tuple(group_map), n, steps)
    env = _make(names, group_map, n, waves, dtype, stats=bool(xo))
    ctx0 = "%s waves=%d xo=%d %s" % ("+".join(names), waves, xo, str(dtype)[6:])
    assert [env.map_of(i) for i in (0, 63, 64, n - 1)] == [names[group_map[g]] for g in (0, 0, 1, (n - 1) // 64)]
    assert_snapshots_equal(env.snapshot(), SetOracleAfterReset(names, group_map, n), ctx0 + " after reset")
    stream = played = None
    if xo:
        stream = _dev(words[0])
        played = torch.zeros((2, n), dtype=torch.int32, device="cuda:0")
    ret, length, prev_done = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    episodes = np.zeros(n, np.int64)
    for k in range(steps):
        ctx = "%s step %d" % (ctx0, k)
        if xo:
            out = env.multi_step(None, ego_pairs=_dev(acts[k][0:2].T), alt_rng=stream, alt_played=played)
        else:
            out = env.multi_step(_dev(acts[k]))
        assert out[0].dtype == dtype
        _check_step(env, out, refs[k], ctx)
        if xo:
            assert np.array_equal(stream.cpu().numpy(), words[k + 1]), ctx
            assert np.array_equal(played.cpu().numpy(), acts[k][2:4]), ctx
            ret, length = oi.stats_step(ret, length, prev_done, refs[k]["reward"])
            assert np.array_equal(bits(env.ep_return.cpu().numpy()), bits(ret)), ctx
            assert np.array_equal(env.ep_length.cpu().numpy(), length), ctx
            prev_done = refs[k]["done"]
        episodes += refs[k]["done"] != 0
    assert episodes.min() >= steps // T, ctx0   # every env auto-reset at every time limit (four times in 120 steps)
    _check_metrics(env, refs, names, ctx0)


@functools.lru_cache(maxsize=None)
def SetOracleAfterReset(names, group_map, n):
    ora = SetOracle(_levels(names), group_map, n)
    ora.reset()
    return ora.snapshot()


THREE = (tuple(TOMATO), (0, 1, 2, 1), 229, 120)


@pytest.mark.parametrize("waves,xo,dtype", [(1, 0, torch.int32), (4, 0, torch.int32), (1, 1, torch.int32),
                                            (4, 1, torch.int32), (4, 0, torch.int8), (4, 1, torch.float32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_three_maps_match_one_oracle_per_map(monkeypatch, waves, xo, dtype):
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    names, gm, n, steps = THREE
    _run(names, gm, n, steps, waves, xo, dtype)


@pytest.mark.parametrize("waves,xo", [(4, 0), (1, 1)])
def test_maps_of_different_sizes(monkeypatch, waves, xo):
    """7 x 7 beside 6 x 5 (another row length, cell count, MAX_PATH -- hence another 1 / MAX_PATH in the
    shaping -- and the Delivery tile on the other wall): the geometry really is per group."""
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    names = ("partial-divider_tomato", "small-tomato")
    a, b = _levels(names)
    assert (a.width, a.height) != (b.width, b.height) and a.delivery != b.delivery and b.width * b.height <= 64
    _run(names, (0, 1), 128, 60, waves, xo)


@pytest.mark.parametrize("waves", [1, 4])
def test_one_map_repeated_equals_the_single_level_batch(monkeypatch, waves):
    from gym_comm_amd.batched import BatchedOvercooked
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    n, steps = 229, 50
    acts, words = _inputs(n, 120)
    kw = dict(device="cuda:0", num_communication=C, fow_radius=RADIUS, auto_reset=True, episode_stats=True,
              waves_per_64=waves)
    one = BatchedOvercooked(_levels(TOMATO[:1])[0], num_envs=n, specialize_level="structure", **kw)
    many = BatchedOvercooked.from_maps(_levels(TOMATO[:2]), group_map=[0, 0, 0, 0], num_envs=n, **kw)
    assert one._L is many._L and one.launch_waves(general=True) == many.launch_waves(general=True) == waves
    assert one.launch_lanes(general=True) == 1
    streams = [_dev(words[0]), _dev(words[0])]
    played = [torch.zeros((2, n), dtype=torch.int32, device="cuda:0") for _ in range(2)]
    for k in range(steps):
        for env, st, pl in zip((one, many), streams, played):
            if k % 2:       # the plain rows and the options in turn (XO = 0 and 1)
                env.multi_step(_dev(acts[k]))
            else:
                env.multi_step(None, ego_pairs=_dev(acts[k][0:2].T), alt_rng=st, alt_played=pl)
        a, b = one.fetch(), many.fetch()
        assert sorted(a) == sorted(b)
        for name in a:      # state, reward, done, comm, obs, timestep, shaped_reward, ep_return, ep_length
            if name != "shaping":       # (the base step's output: neither batch writes it)
                assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), "%s step %d" % (name, k)
        assert torch.equal(streams[0], streams[1]) and torch.equal(played[0], played[1])
    assert torch.equal(one.metrics, many.metrics)
    ma, mb = one.read_metrics(), many.read_metrics()
    assert {c: mb[c] for c in COUNTERS} == ma and mb["per_map"][0] == dict(ma, level=TOMATO[0])
    assert all(mb["per_map"][1][c] == 0 for c in COUNTERS)


def test_masked_reset_observe_and_state_round_trip(monkeypatch):
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    names, gm, n, _ = THREE
    acts, _ = _inputs(n, 120)
    env = _make(names, gm, n, 4)
    ora = SetOracle(_levels(names), gm, n)
    ora.reset()
    for k in range(10):
        env.multi_step(_dev(acts[k]))
        ref = ora.multi_step(acts[k])
    # a mask that cuts through every group: every third env, and the whole tail of the last group
    mask = ((np.arange(n) % 3 == 1) | (np.arange(n) >= 200)).astype(np.int32)
    env.reset(_dev(mask))
    ora.reset(mask)
    assert_snapshots_equal(env.snapshot(), ora.snapshot(), "after the masked reset")
    obs, ts = env.observe()
    want = np.zeros_like(ref["obs"])
    want_ts = np.zeros(n)
    comm = ref["comm"]
    for m, o, ix in ora._each():
        for j, i in enumerate(ix):
            for v in range(2):
                want[v, :, i], want_ts[i] = o.obs(j, v, RADIUS, False, False, C, [int(comm[0, i]), int(comm[1, i])])
    assert np.array_equal(obs.cpu().numpy(), want)
    assert np.array_equal(bits(ts.cpu().numpy()), bits(want_ts))
    # mid-episode: five steps, back to the saved state, the same five steps again
    saved = env.get_state()
    first = []
    for k in range(10, 15):
        env.multi_step(_dev(acts[k]))
        first.append({name: v.copy() for name, v in env.fetch().items()})
    met = env.metrics.clone()
    env.set_state(saved)
    for k in range(10, 15):
        env.multi_step(_dev(acts[k]))
        again = env.fetch()
        for name, v in first[k - 10].items():
            assert np.array_equal(v.view(np.uint8), again[name].view(np.uint8)), "%s step %d" % (name, k)
        _check_step(env, (env.obs, env.timestep, env.shaped_reward, env.done), ora.multi_step(acts[k]), "replayed step %d" % k)
    assert torch.equal(env.metrics, met)


def _arglist():
    return types.SimpleNamespace(level=TOMATO[0], num_agents=2, max_num_timesteps=T, max_num_subtasks=14,
                                 ego_config={}, partner_config={}, num_communication=C, communication_on=True,
                                 ego_led=False, fow_radius=RADIUS, play=False)


def test_vec_env_on_two_maps(monkeypatch):
    from gym_comm_amd.vec_env import OvercookedVecEnv, RandomPartner
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    names, n = TOMATO[:2], 128
    acts, _ = _inputs(229, 120)
    acts = acts[:, :, :n]
    venv = OvercookedVecEnv(_arglist(), n, device="cuda:0", levels=names, seed=5)
    assert [venv._b.map_of(i) for i in (0, 70)] == names
    obs = venv.reset_tensors()
    ora = SetOracle(_levels(names), (0, 1), n)
    ora.reset()
    assert_snapshots_equal(venv._b.snapshot(), ora.snapshot(), "after reset_tensors")
    for k in range(30):
        obs, rew, done = venv.step_tensors(_dev(acts[k][0:2].T))
        full = np.concatenate([acts[k][0:2], venv._act[2:4].cpu().numpy()])       # what the in-kernel partner drew
        ref = ora.multi_step(full)
        _check_step(venv._b, (venv._b.obs, venv._b.timestep, rew, done), ref, "step_tensors %d" % k)
        lo, hi = venv._b._layout["agent1_location"]
        assert np.array_equal(obs["agent1_location"].cpu().numpy(), ref["obs"][0, lo:hi].T)
    # env 70 lives on the second map (its sixth env): its view renders THAT map, as the oracle draws it
    from oracle import oracle
    first, second = _levels(names)
    want = oracle.render_ascii(second.blob, ora.ora[1].snapshot(70 - 64))
    assert str(venv.base_env(70)) == want
    assert want != oracle.render_ascii(first.blob, ora.ora[1].snapshot(70 - 64))      # (the divider shows)
    assert str(venv.base_env(3)) == oracle.render_ascii(first.blob, ora.ora[0].snapshot(3))
    assert venv.get_attr("t", [70])[0] == int(ora.ora[1].snapshot(70 - 64)["t"])
    # a captured 16-step closed loop against the eager one
    outs = []
    for graph in (True, False):
        v = OvercookedVecEnv(_arglist(), n, device="cuda:0", levels=names, seed=5,
                             partner=RandomPartner(C, 9, "cuda:0"))
        v.reset_tensors()
        loop = v.closed_loop(RandomPartner(C, 4, "cuda:0"), graph=graph, steps=16)
        assert not loop.one_launch and (loop.graph is not None) == graph
        loop.step()
        torch.cuda.synchronize()
        outs.append((v._b.fetch(), v._b.metrics.cpu().numpy(), v._act.cpu().numpy()))
    for name, a in outs[0][0].items():
        assert np.array_equal(a.view(np.uint8), outs[1][0][name].view(np.uint8)), name
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert int(outs[0][1][:, 0].sum()) == 16 * n
    with pytest.raises(ValueError):
        from gym_comm_amd.partners import FusedMLPPartner  # noqa: F401
        venv.closed_loop(RandomPartner(C, 4, "cuda:0"), graph=False, one_launch=True)


@pytest.mark.parametrize("flavour", ["level", "generic"])
def test_libraries_without_the_set_kernels_refuse(flavour):
    """Return codes and oc_last_error text only: nothing is launched."""
    from gym_comm_amd import _lib, specialize
    lv = _levels(TOMATO[:1])[0]
    if flavour == "level":
        lv500 = __import__("gym_comm_amd.compiler", fromlist=["x"]).compile_level(TOMATO[0], 2, 500)
        path = specialize.ensure(lv500.blob, geometry=True, compile=False)
        assert path, "build() makes the level library of open-divider_tomato x2"
        L = _lib.load(path)
        assert L.oc_is_specialized() == 2
    else:
        L = _lib.load()
        assert L.oc_is_specialized() == 0
    i32p = ctypes.POINTER(ctypes.c_int32)
    blob = np.ascontiguousarray(lv.blob, dtype=np.int32)
    ptrs = (i32p * 1)(blob.ctypes.data_as(i32p))
    sizes = np.array([blob.size], np.int32)
    h = ctypes.c_void_p()
    rc = L.oc_mapset_create(ptrs, sizes.ctypes.data_as(i32p), 1, ctypes.byref(h))
    assert rc == -1 and not h.value
    assert b"structure library" in L._oc_last_error()
    assert L.oc_mapset_multi_step_waves(4096, 0, 0) == 0


def test_structure_library_refusals_name_the_blob():
    from gym_comm_amd import _lib, compiler, specialize
    lv = _levels(TOMATO[:1])[0]
    other = compiler.compile_level("full-divider_salad", 2, T)
    three = compiler.compile_level("partial-divider_tl", 3, T)
    _, L = specialize.load_for(lv.blob, "structure")
    i32p = ctypes.POINTER(ctypes.c_int32)

    def create(lvs, k=None):
        blobs = [np.ascontiguousarray(m.blob, dtype=np.int32) for m in lvs]
        ptrs = (i32p * max(len(blobs), 1))(*[b.ctypes.data_as(i32p) for b in blobs])
        sizes = np.array([b.size for b in blobs] or [0], np.int32)
        h = ctypes.c_void_p()
        rc = L.oc_mapset_create(ptrs, sizes.ctypes.data_as(i32p), len(blobs) if k is None else k, ctypes.byref(h))
        return rc, h, L._oc_last_error().decode()

    rc, h, msg = create([lv], k=0)
    assert rc == -1 and "k < 1" in msg
    rc, h, msg = create([lv, lv, other])
    assert rc == -1 and "blob 2" in msg and "structure" in msg
    rc, h, msg = create([lv, three])
    assert rc == -1 and "blob 1" in msg
    rc, h, msg = create([lv, _levels(TOMATO[1:2])[0]])
    assert rc == 0 and h.value
    assert L.oc_mapset_destroy(h) == 0
