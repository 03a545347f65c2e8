"""-m gpu: the fused rollout buffer (include/oc_rollout.h; ``RolloutSink(fused=True)``).

  1. recording: the fused sink and the torch sink, fed the same tensors, hold the same bits after
     every step -- a ring that wraps twice, two adds in a row, every observation element type,
     sizes around the wave and the workgroup;
  2. the same inside ONE captured graph (a linear one), replayed;
  3. through the partner protocol (``RecurrentPolicyPartner`` in ``OvercookedVecEnv``, eager and
     captured), against the torch sink and the oracle, then ``finish_rollout``;
  4. returns / advantages against the float32 numpy loop of tests/rollout_ref.py, bit for bit:
     IEEE float32, one rounding per operation, the same order, nothing contracted, inputs on a
     1/1024 grid so that no intermediate comes near the denormal range -- equality is derived,
     not a tolerance;
  5. recording on every path of ``k_rollout_add`` that the launch policy can choose -- several rows
     per workgroup, a second and third block of eight, a group that holds observation rows and
     extra rows, the stride over envs -- each case reading its launch through
     ``oc_rollout_add_plan`` and asserting the property it exists for BEFORE it launches; counter
     words outside 0..T-1;
  6. returns / advantages over more than one block of eight steps: a short second block, the ring's
     wrap inside the first block, on a block boundary and in a later block, partly filled buffers,
     counter words out of range, and (gamma, lambda) pairs at which float32(gamma * lambda in
     double) is not the float32 product of the rounded factors.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rollout_ref

pytestmark = pytest.mark.gpu

FIELDS = ("obs", "timestep", "actions", "log_probs", "values", "rewards", "episode_starts", "dones",
          "pos", "last", "count")


def _bits(t):
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b, where):
    for f in FIELDS:
        assert torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (f, where)
    assert int(a.ticket.item()) == 0, where


def _inputs(k, n, F, dt, gen):
    """k steps' worth of what add / add_reward take, seeded, on the device."""
    ri = lambda lo, hi, *shape: torch.randint(lo, hi, shape, generator=gen)
    if dt == torch.float32:
        rows = torch.randn((k, F, n), generator=gen)
    else:
        lo, hi = (-128, 128) if dt == torch.int8 else (-100000, 100000)
        rows = ri(lo, hi, k, F, n).to(dt)
    d = dict(rows=rows, timestep=torch.rand((k, n), generator=gen, dtype=torch.float64) * 100,
             move=ri(0, 4, k, n).to(torch.int32), comm=ri(0, 10, k, n).to(torch.int32),
             log_prob=torch.randn((k, n), generator=gen), value=torch.randn((k, n), generator=gen),
             episode_start=ri(0, 2, k, n).to(torch.float32),
             reward=torch.randn((k, n), generator=gen, dtype=torch.float64), done=ri(0, 2, k, n).to(torch.int32))
    return {key: t.cuda() for key, t in d.items()}


def _add(sink, d, k, value=True):
    sink.add(d["rows"][k], d["timestep"][k], d["move"][k], d["comm"][k], d["log_prob"][k],
             d["value"][k] if value else None, d["episode_start"][k])


def _pair(T, n, F, dt):
    from gym_comm_amd.vec_env import RolloutSink
    fused = RolloutSink(T, n, F, obs_dtype=dt, fused=True)
    plain = RolloutSink(T, n, F, obs_dtype=dt)
    assert fused.fused and not plain.fused
    return fused, plain


# ---- 1. recording ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.int32, torch.int8, torch.float32], ids=["int32", "int8", "float32"])
@pytest.mark.parametrize("F", [1, 29])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fused_recording_equals_torch_recording(n, F, dt):
    K, T = 7, 3
    fused, plain = _pair(T, n, F, dt)
    d = _inputs(K + 2, n, F, dt, torch.Generator().manual_seed(1000 * n + F))
    extra = {2: K, 5: K + 1}                   # on these steps: add, add again, then the reward
    for k in range(K):
        for sink in (fused, plain):
            _add(sink, d, k)
            if k in extra:
                _add(sink, d, extra[k])
            sink.add_reward(d["reward"][k], d["done"][k])
        _same(fused, plain, k)
    assert fused.steps() == K + 2 and int(fused.pos.item()) == (K + 2) % T      # the ring wrapped twice
    fused.reset()
    assert fused.steps() == 0 and int(fused.pos.item()) == 0 and int(fused.ticket.item()) == 0


@pytest.mark.parametrize("case", ["no value", "int64 actions", "strided rows", "float64 log_prob"])
def test_fused_recording_converts_what_the_torch_path_converts(case):
    K, T, n, F = 5, 3, 130, 4
    fused, plain = _pair(T, n, F, torch.float32)
    d = _inputs(K, n, F, torch.float32, torch.Generator().manual_seed(7))
    if case == "int64 actions":
        d["move"], d["comm"] = d["move"].to(torch.int64), d["comm"].to(torch.int64)
    elif case == "strided rows":               # every other row of a tensor twice as tall
        tall = torch.randn((K, 2 * F, n), generator=torch.Generator().manual_seed(8)).cuda()
        d["rows"] = tall[:, ::2]
        assert not d["rows"][0].is_contiguous()
    elif case == "float64 log_prob":
        d["log_prob"] = d["log_prob"].to(torch.float64) * (1 + 2.0 ** -40)     # rounds on the way in
    for sink in (fused, plain):                # what value=None must leave alone
        sink.values.fill_(-7.5)
    for k in range(K):
        for sink in (fused, plain):
            _add(sink, d, k, value=case != "no value")
            sink.add_reward(d["reward"][k], d["done"][k])
        _same(fused, plain, k)
    if case == "no value":
        assert bool((fused.values == -7.5).all())


# ---- 2. inside a captured graph -------------------------------------------------------------------
@pytest.mark.parametrize("n,F", [(130, 6), (3585, 29)], ids=["n130-F6", "two-rows-per-group"])
def test_fused_recording_inside_a_captured_graph(n, F):
    from gym_comm_amd.vec_env import RolloutSink
    per, replays, T = 4, 3, 5
    fused, plain = _pair(T, n, F, torch.int32)
    if n > 256:                                # the ticket drawn by a few hundred workgroups under replay
        gx, groups, pg = _plan(fused)
        assert pg == 2 and _straddles(F, pg) and 200 <= gx * groups <= 512, (gx, groups, pg)
    gen = torch.Generator().manual_seed(21)
    d = _inputs(per * replays, n, F, torch.int32, gen)
    static = {key: t[:per].clone() for key, t in d.items()}
    warm = RolloutSink(T, n, F, obs_dtype=torch.int32, fused=True)          # code objects load outside the capture
    _add(warm, static, 0)
    warm.add_reward(static["reward"][0], static["done"][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):              # one stream: a linear graph of 8 kernel nodes
        for j in range(per):
            _add(fused, static, j)
            fused.add_reward(static["reward"][j], static["done"][j])
    assert fused.steps() == 0                  # capturing ran nothing
    for rep in range(replays):
        for key, t in static.items():
            t.copy_(d[key][rep * per:(rep + 1) * per])
        graph.replay()
    torch.cuda.synchronize()
    for k in range(per * replays):
        _add(plain, d, k)
        plain.add_reward(d["reward"][k], d["done"][k])
    _same(fused, plain, "after %d replays" % replays)
    assert fused.steps() == 12 and int(fused.pos.item()) == 12 % T


# ---- 3. through the partner protocol --------------------------------------------------------------
S, C, TMAX = 3, 2, 25
NF = 22 + S + 2 * C
HID = 32


class LSTMPolicy(torch.nn.Module):
    """The policy of tests/test_recurrent_partner_gpu.py: obs rows (+ timestep) -> LSTMCell -> move /
    comm logits and a value."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.cell = torch.nn.LSTMCell(NF + 1, HID)
        self.move = torch.nn.Linear(HID, 4)
        self.comm = torch.nn.Linear(HID, C)
        self.val = torch.nn.Linear(HID, 1)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.8)

    def forward(self, obs, state, episode_start):
        x = torch.cat([obs.rows.T, obs.timestep.to(torch.float32).unsqueeze(1)], dim=1)
        keep = (1.0 - episode_start).unsqueeze(1)
        h, c = self.cell(x, (state[0] * keep, state[1] * keep))
        return self.move(h), self.comm(h), (h, c), self.val(h)


def _args():
    return SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=TMAX, ego_config={},
                           partner_config={}, num_communication=C, communication_on=True, ego_led=False,
                           fow_radius=2)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_fused_sink_through_the_partner_protocol(use_graph, oracle_lib):
    from gym_comm_amd.vec_env import OvercookedVecEnv, RecurrentPolicyPartner, RolloutSink
    n, K = 64, 60
    gen = torch.Generator(device="cuda").manual_seed(11)
    ego = torch.stack([torch.randint(0, 4, (K, n), generator=gen, device="cuda"),
                       torch.randint(0, C, (K, n), generator=gen, device="cuda")], dim=2).to(torch.int32)
    runs = {}
    for fused in (True, False):
        pol = LSTMPolicy(seed=3).cuda()
        sink = RolloutSink(K, n, NF, obs_dtype=torch.float32, fused=fused)
        state = (torch.zeros(n, HID, device="cuda"), torch.zeros(n, HID, device="cuda"))
        partner = RecurrentPolicyPartner(pol, state, sample=True, sink=sink)
        venv = OvercookedVecEnv(_args(), n, partner=partner, seed=5, obs_dtype=torch.float32, use_graph=use_graph)
        torch.cuda.manual_seed(1234)
        venv.reset_tensors()
        for k in range(K):
            venv.step_tensors(ego[k].contiguous())
        assert sink.steps() == K and sink.full()
        runs[fused] = (sink, partner, venv)
    (fs, fp, fv), (ps, pp, pv) = runs[True], runs[False]
    _same(fs, ps, "after %d steps" % K)
    for a, b in zip(fp.state + (fp.episode_start, fp.log_prob, fp.value),
                    pp.state + (pp.episode_start, pp.log_prob, pp.value)):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(fv._b.state, pv._b.state) and torch.equal(_bits(fv._b.obs), _bits(pv._b.obs))
    assert int(fs.dones.sum().item()) >= 2 * n          # every env started over at least twice
    # the env side against the oracle, fed the recorded actions
    ora = oracle_lib.OracleBatch(fv._b.level.blob, n, threads=4)
    comm = np.zeros((2, n), np.int32)
    act, eg = fs.actions.cpu().numpy(), ego.cpu().numpy()
    rew, done = fs.rewards.cpu().numpy(), fs.dones.cpu().numpy()
    for k in range(K):
        a4 = np.stack([eg[k, :, 0], eg[k, :, 1], act[k, 0], act[k, 1]]).astype(np.int32)
        _, _, ro, do = ora.multi_step(a4, comm, 2, 0, C, auto_reset=True)
        assert np.array_equal(do, done[k]), k
        assert np.array_equal(ro.view(np.uint64), rew[k].view(np.uint64)), k
    # returns and advantages: kernel, torch restatement and the numpy reference
    fa, fr = fp.finish_rollout()
    pa, pr = pp.finish_rollout()
    assert fa is fs.advantages and fr is fs.returns and fa.shape == (K, n) and fa.dtype == torch.float32
    assert torch.equal(_bits(fa), _bits(pa)) and torch.equal(_bits(fr), _bits(pr))
    ea, er = rollout_ref.gae(rew, fs.values.cpu().numpy(), fs.episode_starts.cpu().numpy(), fp.value.cpu().numpy(),
                             fp.episode_start.cpu().numpy(), 0.99, 0.95, np.float32)
    assert np.array_equal(fa.cpu().numpy().view(np.int32), ea.view(np.int32))
    assert np.array_equal(fr.cpu().numpy().view(np.int32), er.view(np.int32))
    assert fs.steps() == K                               # finish_rollout does not reset the sink


# ---- 4. returns and advantages against the float32 reference, bit for bit ----------------------------
SENTINEL = 777.25


def _grid(gen, *shape):
    """multiples of 1/1024 in [-4, 4]"""
    return torch.randint(-4096, 4097, shape, generator=gen).to(torch.float64) / 1024


def _filled_sink(T, n, state, gen):
    """A fused sink in one of three states, and its chronological (rewards, values, episode_starts)."""
    from gym_comm_amd.vec_env import RolloutSink
    sink = RolloutSink(T, n, 1, obs_dtype=torch.float32, fused=True)
    steps = {"full": T, "wrapped": T + 3, "partial": T - 1}[state]
    r, v = _grid(gen, steps, n), _grid(gen, steps, n).to(torch.float32)
    es = (torch.rand((steps, n), generator=gen) < 0.3).to(torch.float32)
    if state == "wrapped":                      # through real add calls: the counters are the kernel's own
        rows, ts, z = torch.zeros((1, n), device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"), \
            torch.zeros(n, dtype=torch.int32, device="cuda")
        for k in range(steps):
            sink.add(rows, ts, z, z, v[k].cuda(), v[k].cuda(), es[k].cuda())
            sink.add_reward(r[k].cuda(), z)
        assert sink.steps() == T + 3 and int(sink.pos.item()) == 3 % T
    else:
        sink.rewards[:steps] = r.cuda()
        sink.values[:steps] = v.cuda()
        sink.episode_starts[:steps] = es.cuda()
        sink.count.fill_(steps)
        sink.pos.fill_(steps % T)
    sink.advantages.fill_(SENTINEL)
    sink.returns.fill_(SENTINEL)
    return sink


# exactly full and wrapped at every T; partly filled (count = T - 1) where there are two slots
GAE_CASES = [(n, T, state) for n in (1, 64, 65, 200) for T in (1, 2, 8) for state in ("full", "wrapped", "partial")
             if not (state == "partial" and T < 2)]


@pytest.mark.parametrize("n,T,state", GAE_CASES, ids=["n%d-T%d-%s" % c for c in GAE_CASES])
def test_gae_kernel_equals_float32_reference_bit_for_bit(n, T, state):
    gen = torch.Generator().manual_seed(100 * n + 10 * T + len(state))
    sink = _filled_sink(T, n, state, gen)
    lv = _grid(gen, n).to(torch.float32)
    ld = torch.randint(0, 2, (n,), generator=gen).to(torch.float32)
    adv, ret = sink.compute_returns_and_advantage(lv.cuda(), ld.cuda(), gamma=0.99, gae_lambda=0.95)
    assert adv is sink.advantages and ret is sink.returns
    pos, count = int(sink.pos.item()), sink.steps()
    order = rollout_ref.slots(pos, count, T)
    assert len(order) == (T - 1 if state == "partial" else T)
    r, v, es = (t.cpu().numpy()[order] for t in (sink.rewards, sink.values, sink.episode_starts))
    ea, er = rollout_ref.gae(r, v, es, lv.numpy(), ld.numpy(), 0.99, 0.95, np.float32)
    want_a = np.full((T, n), SENTINEL, np.float32)
    want_r = np.full((T, n), SENTINEL, np.float32)
    want_a[order], want_r[order] = ea, er                # slots that hold no step keep the sentinel
    got_a, got_r = adv.cpu().numpy(), ret.cpu().numpy()
    assert np.array_equal(got_a.view(np.int32), want_a.view(np.int32))
    assert np.array_equal(got_r.view(np.int32), want_r.view(np.int32))
    if state == "partial":
        assert (got_a[T - 1] == SENTINEL).all() and (got_r[T - 1] == SENTINEL).all()
    # last_values / last_dones of another dtype are converted first: the same bits
    sink.advantages.fill_(SENTINEL)
    sink.returns.fill_(SENTINEL)
    adv2, ret2 = sink.compute_returns_and_advantage(lv.to(torch.float64).cuda(), ld.to(torch.int32).cuda(),
                                                    gamma=0.99, gae_lambda=0.95)
    assert np.array_equal(adv2.cpu().numpy().view(np.int32), want_a.view(np.int32))
    assert np.array_equal(ret2.cpu().numpy().view(np.int32), want_r.view(np.int32))
    assert sink.steps() == count and int(sink.pos.item()) == pos      # the counters are only read


def test_gae_kernel_equals_closed_form_on_integers():
    from gym_comm_amd.vec_env import RolloutSink
    r, v, es, lv, ld = rollout_ref.integer_case()
    T, n = v.shape
    sink = RolloutSink(T, n, 1, obs_dtype=torch.float32, fused=True)
    sink.rewards.copy_(torch.from_numpy(r))
    sink.values.copy_(torch.from_numpy(v))
    sink.episode_starts.copy_(torch.from_numpy(es))
    sink.count.fill_(T)
    adv, ret = sink.compute_returns_and_advantage(torch.from_numpy(lv).cuda(), torch.from_numpy(ld).cuda(),
                                                  gamma=1.0, gae_lambda=1.0)
    ac, rc = rollout_ref.closed_form(r, v, es, lv, ld)
    assert (adv.cpu().numpy() == ac).all() and (ret.cpu().numpy() == rc).all()


# ---- 5. recording, on every path the launch policy can choose -------------------------------------
def _plan(sink):
    """(gridDim.x, groups, per_group) of the launch ``oc_rollout_add`` makes for this sink."""
    plan = (ctypes.c_int32 * 3)(-1, -1, -1)
    assert sink._L.oc_rollout_add_plan(ctypes.byref(sink._buf), plan) == 0, sink._L.oc_rollout_last_error()
    return tuple(plan)


def _straddles(F, pg):
    """some group holds the last observation row(s) AND the first extra row"""
    return any(k * pg < F < (k + 1) * pg for k in range(F))


# path -> (n, F, the property of the launch the case exists for); the smallest shapes found that have it
PATHS = {
    "two-rows-straddling": (3585, 29, lambda gx, groups, pg, n, F: pg == 2 and _straddles(F, pg)),
    "three-to-seven-ragged": (2305, 120, lambda gx, groups, pg, n, F: 3 <= pg <= 7 and (F + 7) % pg != 0),
    "second-block-partial": (2400, 497, lambda gx, groups, pg, n, F: 8 < pg < 16 and pg % 8 != 0 and
                             _straddles(F, pg) and (F + 7) % pg != 0),
    "three-blocks": (65536, 29, lambda gx, groups, pg, n, F: pg > 16 and groups == 2),
    "grid-stride-uneven": (25601, 29, lambda gx, groups, pg, n, F: gx < (n + 255) // 256 < 2 * gx and n % 256 != 0),
    "one-group-and-a-stride": (131073, 1, lambda gx, groups, pg, n, F: groups == 1 and gx < (n + 255) // 256),
}
PATH_CASES = [(path, torch.int32, True) for path in PATHS] + \
             [(path, torch.int8, True) for path in ("second-block-partial", "three-blocks", "grid-stride-uneven")] + \
             [("two-rows-straddling", torch.float32, True), ("three-to-seven-ragged", torch.int32, False)]
PATTERN = 91                                     # what every buffer tensor holds before the first step


def _fill_pattern(*sinks):
    """A row that is never stored cannot pass as a zero, and a reward row that is not zeroed shows."""
    for sink in sinks:
        for f in FIELDS[:8]:
            getattr(sink, f).fill_(PATTERN)


@pytest.mark.parametrize("path,dt,value", PATH_CASES,
                         ids=["%s-%s%s" % (p, str(d).split(".")[1], "" if v else "-no-value") for p, d, v in PATH_CASES])
def test_fused_recording_on_every_path_of_the_add_kernel(path, dt, value):
    n, F, has_property = PATHS[path]
    K, T = 5, 2                                  # the ring wraps twice
    fused, plain = _pair(T, n, F, dt)
    plan = _plan(fused)
    assert has_property(*plan, n, F), (path, plan)       # the case reaches the path it is named for
    _fill_pattern(fused, plain)
    d = _inputs(K + 1, n, F, dt, torch.Generator().manual_seed(n + F))
    for k in range(K):
        for sink in (fused, plain):
            _add(sink, d, k, value=value)
            if k == 1:                           # add, add again, then the reward
                _add(sink, d, K, value=value)
            sink.add_reward(d["reward"][k], d["done"][k])
        _same(fused, plain, (path, k))
    assert fused.steps() == K + 1 and int(fused.pos.item()) == (K + 1) % T
    if not value:
        assert bool((fused.values == PATTERN).all())


@pytest.mark.parametrize("word", ["T+1", "-1", "2T"])
def test_add_takes_a_position_outside_the_ring_modulo_T(word):
    T, n, F = 3, 300, 2
    bad = {"T+1": T + 1, "-1": -1, "2T": 2 * T}[word]
    slot = bad % T                               # non-negative
    assert slot == {"T+1": 1, "-1": 2, "2T": 0}[word]
    fused, plain = _pair(T, n, F, torch.int32)
    _fill_pattern(fused, plain)
    d = _inputs(3, n, F, torch.int32, torch.Generator().manual_seed(5))
    for sink in (fused, plain):                  # one ordinary step first: count is not 0
        _add(sink, d, 0)
        sink.add_reward(d["reward"][0], d["done"][0])
    fused.pos.fill_(bad)
    plain.pos.fill_(slot)                        # the torch sink only ever sees the reduced value
    for sink in (fused, plain):
        _add(sink, d, 1)
    _same(fused, plain, "after the add")
    assert (int(fused.last.item()), int(fused.pos.item()), fused.steps()) == (slot, (slot + 1) % T, 2)
    for sink in (fused, plain):
        sink.add_reward(d["reward"][1], d["done"][1])
        _add(sink, d, 2)
        sink.add_reward(d["reward"][2], d["done"][2])
    _same(fused, plain, "after the next step")


@pytest.mark.parametrize("word", ["T+1", "-1"])
def test_add_reward_takes_a_last_outside_the_ring_modulo_T(word):
    T, n, F = 3, 300, 2
    bad = {"T+1": T + 1, "-1": -1}[word]
    slot = bad % T
    fused, plain = _pair(T, n, F, torch.int32)
    _fill_pattern(fused, plain)
    d = _inputs(2, n, F, torch.int32, torch.Generator().manual_seed(6))
    for sink in (fused, plain):
        _add(sink, d, 0)                         # slot 0; the reward below goes elsewhere, onto the pattern
    fused.last.fill_(bad)
    plain.last.fill_(slot)
    for sink in (fused, plain):
        sink.add_reward(d["reward"][1], d["done"][1])
    assert int(fused.last.item()) == bad         # add_reward only reads the word
    fused.last.fill_(slot)
    _same(fused, plain, word)
    want = d["reward"][1] + PATTERN
    assert slot != 0 and torch.equal(_bits(fused.rewards[slot]), _bits(want))
    assert torch.equal(fused.dones[slot], d["done"][1])


# ---- 6. returns and advantages: blocks of eight, the ring and the counters ---------------------------
def _ring_cases():
    cases = []
    for T in (9, 16, 17, 23):
        for n in (1, 65):
            cases.append((n, T, 0, T, "full"))
            for pos in sorted({1, 7, 8, 9, T - 1}):
                if pos < T:
                    # the wrap inside the first block, on the block boundary, in a later block
                    cases.append((n, T, pos, T + pos, "wrapped"))
                    cases.append((n, T, pos, pos, "partial"))
    cases.append((65, 17, 2, 3 * 17 + 2, "wrapped"))
    T = 9                                        # counter words out of range: (pos, count) as the sink holds them
    cases += [(65, T, T + 3, T, "pos=T+3"), (65, T, -1, T, "pos=-1"), (65, T, 0, 2 ** 40, "count=2^40"),
              (65, T, 4, -5, "count=-5"), (65, T, 4, 0, "count=0")]
    return [c + (0.99, 0.95) for c in cases]


# two of the cases again, at pairs that tell float32(gamma * lambda in double) from the float32 product
SHARP_PAIRS = ((0.9, 0.8), (0.995, 0.97))
RING_CASES = _ring_cases() + [c + pair for pair in SHARP_PAIRS
                              for c in ((65, 17, 9, 17 + 9, "wrapped"), (65, 23, 9, 9, "partial"))]


@pytest.mark.parametrize("n,T,pos,count,state,gamma,lam", RING_CASES,
                         ids=["n%d-T%d-pos%d-count%d-%s-g%s-l%s" % c for c in RING_CASES])
def test_gae_kernel_over_blocks_ring_and_counters_bit_for_bit(n, T, pos, count, state, gamma, lam):
    from gym_comm_amd.vec_env import RolloutSink
    gen = torch.Generator().manual_seed(1000 * T + 10 * n + (pos % 7))
    sink = RolloutSink(T, n, 1, obs_dtype=torch.float32, fused=True)
    r, v = _grid(gen, T, n), _grid(gen, T, n).to(torch.float32)       # every slot holds numbers
    es = (torch.rand((T, n), generator=gen) < 0.3).to(torch.float32)
    lv = _grid(gen, n).to(torch.float32)
    ld = torch.randint(0, 2, (n,), generator=gen).to(torch.float32)
    sink.rewards.copy_(r)
    sink.values.copy_(v)
    sink.episode_starts.copy_(es)
    sink.pos.fill_(pos)
    sink.count.fill_(count)
    sink.advantages.fill_(SENTINEL)
    sink.returns.fill_(SENTINEL)
    adv, ret = sink.compute_returns_and_advantage(lv.cuda(), ld.cuda(), gamma=gamma, gae_lambda=lam)
    # the reference at the values the header reduces the words to
    L = max(0, min(count, T))
    order = np.array(rollout_ref.slots(pos % T, L, T), dtype=np.intp)
    assert len(order) == L == {"full": T, "wrapped": T, "partial": pos, "pos=T+3": T, "pos=-1": T,
                               "count=2^40": T, "count=-5": 0, "count=0": 0}[state]
    data = (r.numpy()[order], v.numpy()[order], es.numpy()[order], lv.numpy(), ld.numpy())
    ea, er = rollout_ref.gae(*data, gamma, lam, np.float32)
    want_a = np.full((T, n), SENTINEL, np.float32)
    want_r = np.full((T, n), SENTINEL, np.float32)
    want_a[order], want_r[order] = ea, er                # slots that hold no step keep the sentinel
    got_a, got_r = adv.cpu().numpy(), ret.cpu().numpy()
    assert np.array_equal(got_a.view(np.int32), want_a.view(np.int32))
    assert np.array_equal(got_r.view(np.int32), want_r.view(np.int32))
    if state == "partial":                               # every slot from count upward
        assert (got_a[count:] == SENTINEL).all() and (got_r[count:] == SENTINEL).all()
        assert not (got_a[:count] == SENTINEL).any()
    if L == 0:
        assert (got_a == SENTINEL).all() and (got_r == SENTINEL).all()
    assert int(sink.pos.item()) == pos and int(sink.count.item()) == count      # the counters are only read
    if (gamma, lam) in SHARP_PAIRS:
        # the pair tells the two products apart, and the planted mutant -- the product formed in
        # float32 -- gives other advantages on this very data: the comparison above rejects it
        mutant = rollout_ref.gl_float32_product(gamma, lam)
        assert np.float32(gamma * lam) != mutant
        ma, _ = rollout_ref.gae(*data, gamma, lam, np.float32, gl=mutant)
        assert (ma.view(np.int32) != ea.view(np.int32)).any()
    else:
        assert np.float32(gamma * lam) == rollout_ref.gl_float32_product(gamma, lam)
