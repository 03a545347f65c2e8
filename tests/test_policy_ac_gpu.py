"""-m gpu: the actor-critic form of the fused MLP policy (include/oc_policy.h: oc_policy_mlp_ac;
``FusedActorCriticPartner``) env by env against tests/policy_ac_ref.py.

The same policy as the plain kernel bit for bit (pairs, logits, streams); the value within
policy_ref.logit_bound of its row; the log-probability of the action the kernel itself wrote within
policy_ac_ref.log_prob_bound -- both bounds tight enough that planted mutants of the reference are
rejected on the same data; the ``given`` mode; nothing stored past n; and the seat: recording
through a fused ``RolloutSink``, eager and as one captured 16-step closed loop."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import policy_ac_ref as ar  # noqa: E402
import policy_ref as pr  # noqa: E402
import rollout_ref  # noqa: E402

pytestmark = pytest.mark.gpu

OT = {"int32": 0, "int8": 1, "float32": 2}
WORST = {"value": 0.0, "log_prob": 0.0}          # largest |kernel - reference| / bound seen in this session
SENT = -0x5A5A5A5B
GUARD = 257


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


class Player:
    """One player of a raw oc_policy_mlp_ac launch: every output a view at the front of a larger
    buffer whose tail keeps a sentinel."""

    def __init__(self, F, C, odt, n, seed, scale, sample, rng_seed):
        from gym_comm_amd.vec_env import FusedActorCriticPartner, FusedMLPPartner
        self.pol = ar.make_actor_critic(F, C, seed, scale).cuda()
        self.w, self.wv, self.bv = ar.weights(self.pol)
        self.ac = FusedActorCriticPartner(self.pol, sample=sample, seed=rng_seed)      # packed WITH the value row
        self.plain = FusedMLPPartner(self.pol, sample=sample, seed=rng_seed, keep_logits=True)   # and without
        self.rows_np = ar.make_rows(F, n, odt, 100 * F + C + seed)
        self.rows = torch.from_numpy(self.rows_np).cuda()
        self.n, self.C, self.sample = n, C, sample
        i32 = lambda k: torch.full((k + GUARD,), SENT, dtype=torch.int32, device="cuda")  # noqa: E731
        f32 = lambda k: torch.full((k + GUARD,), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
        self.pairs, self.move, self.comm = i32(2 * n), i32(n), i32(n)
        self.log_prob, self.value, self.logits = f32(n), f32(n), f32((4 + C) * n)
        self.plain._buffers(n)
        self.rng = i32(2 * n)
        self.rng[:2 * n] = self.plain._rng.reshape(-1)

    def struct(self, _lib, given=None, pairs=True):
        w = self.ac._w
        return _lib.PolicyAcPlayer(
            _lib.PolicyPlayer(self.rows.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(),
                              self.rng.data_ptr() if self.sample else None,
                              self.pairs.data_ptr() if pairs else None, self.logits.data_ptr()),
            None if given is None else given.data_ptr(), self.move.data_ptr(), self.comm.data_ptr(),
            self.log_prob.data_ptr(), self.value.data_ptr())

    def guards_intact(self):
        n, C = self.n, self.C
        for t, k in ((self.pairs, 2 * n), (self.move, n), (self.comm, n), (self.rng, 2 * n)):
            assert (t[k:] == SENT).all()
        for t, k in ((self.log_prob, n), (self.value, n), (self.logits, (4 + C) * n)):
            assert torch.isnan(t[k:]).all() and not torch.isnan(t[:k]).any()


def _launch_ac(players, ts, F, C, odt, n, given=None, pairs=True):
    from gym_comm_amd import _lib
    L = _lib.load(lib="policy")
    arr = (_lib.PolicyAcPlayer * len(players))(*[p.struct(_lib, given, pairs) for p in players])
    rc = L.oc_policy_mlp_ac(arr, len(players), ts.data_ptr(), F, C, OT[odt], n,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.oc_policy_last_error()
    torch.cuda.synchronize()


def _check_value(p, got, tsn, tag, mutants):
    ref = ar.ref_value(p.w, p.wv, p.bv, p.rows_np, tsn)
    bound = ar.value_bound(p.w, p.wv, p.bv, p.rows_np, tsn)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-30)).max())
    WORST["value"] = max(WORST["value"], ratio)
    print("policy-ac value %s: max err %.3g, max bound %.3g, max err/bound %.3f (session max %.3f)"
          % (tag, err.max(), bound.max(), ratio, WORST["value"]))
    assert (err <= bound).all(), (tag, np.argwhere(err > bound)[:5].tolist())
    if mutants:
        logits = pr.ref_logits(*p.w, p.rows_np, tsn)
        planted = {"value read from a logit row": logits[0],
                   "value read from the first comm row": logits[4],
                   "value without the row-sum fold": ar.ref_value(p.w, p.wv, p.bv, p.rows_np, tsn, fold=False)}
        for name, m in planted.items():
            assert (np.abs(got - m) > bound).any(), "the value bound lets a planted bug through: " + name


def _check_log_prob(p, got, actions, tsn, tag, mutants):
    ref, terms = ar.ref_log_prob(p.w, p.rows_np, tsn, actions)
    bound = ar.log_prob_bound(p.w, p.rows_np, tsn, actions)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-30)).max())
    WORST["log_prob"] = max(WORST["log_prob"], ratio)
    print("policy-ac log_prob %s: max err %.3g, max bound %.3g, max err/bound %.3f (session max %.3f)"
          % (tag, err.max(), bound.max(), ratio, WORST["log_prob"]))
    assert (err <= bound).all(), (tag, np.argwhere(err > bound)[:5].tolist())
    if mutants:
        logits = pr.ref_logits(*p.w, p.rows_np, tsn)
        idx = np.arange(p.n)
        raw = [logits[lo:hi][actions[:, col], idx] - logits[lo:hi].max(axis=0) for col, (lo, hi) in
               enumerate(((0, 4), (4, 4 + p.C)))]
        planted = {"no normaliser": raw[0] + raw[1], "base-2 result": ref / pr.LN2}
        if p.C > 1:          # (with one comm channel the comm head's term is exactly 0)
            planted["only the move head's term"] = terms[0]
        for name, m in planted.items():
            assert (np.abs(got - m) > bound).any(), "the log-prob bound lets a planted bug through: " + name


# (F, C, row type, n, players, OC_POLICY_WG32, weight scale, sampled): k-steps 1 / 2 / 3 / 3 and CMAX
# 4 / 4 / 8 / 16; a lone lane on a clamped env, a second wave with one env, ragged multi-workgroup
# batches; scales as tests/test_policy_reference_gpu.py (x32: hidden units saturate)
CASES = [
    (7, 1, "int8", 1, 1, 0, 1, True),
    (7, 1, "float32", 97, 2, 0, 4, False),
    (29, 2, "float32", 33, 1, 0, 1, True),
    (29, 2, "int32", 200, 2, 0, 4, True),
    (29, 2, "int8", 97, 1, 1, 32, False),
    (35, 5, "int32", 1, 2, 0, 4, False),
    (35, 5, "int8", 33, 2, 1, 4, True),
    (35, 5, "float32", 200, 1, 0, 32, True),
    (46, 16, "int8", 97, 1, 0, 1, True),
    (46, 16, "float32", 33, 1, 0, 4, False),
    (46, 16, "int32", 200, 2, 0, 1, True),
    (46, 16, "int32", 1, 1, 0, 32, True),
]


@pytest.mark.parametrize("F,C,odt,n,players,wg32,scale,sample", CASES,
                         ids=["F%d-C%d-%s-n%d-p%d-wg%d-x%d-%s" % (c[0], c[1], c[2], c[3], c[4], 32 if c[5] else 64, c[6],
                                                                  "sampled" if c[7] else "greedy") for c in CASES])
def test_same_policy_as_the_plain_kernel_with_value_and_log_prob(F, C, odt, n, players, wg32, scale, sample, monkeypatch):
    from gym_comm_amd.vec_env import FusedMLPPartner
    if wg32:
        monkeypatch.setenv("OC_POLICY_WG32", "1")
    else:
        monkeypatch.delenv("OC_POLICY_WG32", raising=False)
    ps = [Player(F, C, odt, n, 20 + 7 * k + F, scale, sample, 70 + k) for k in range(players)]
    ts = torch.from_numpy(ar.make_timesteps(n, 333, F + n)).cuda()
    tsn = ts.cpu().numpy()
    # the logit rows of both packings are the same bits
    for p in ps:
        other = [l for l in range(64) if l & 31 != 8]
        assert torch.equal(p.ac._w[0], p.plain._w[0])
        assert torch.equal(p.ac._w[1].view(4, 64, 8)[:, other], p.plain._w[1].view(4, 64, 8)[:, other])
        keep = torch.ones((64, 16), dtype=torch.bool, device="cuda")
        keep[:32, 4] = False
        assert torch.equal(_bits(p.ac._w[2])[keep], _bits(p.plain._w[2])[keep])
    for launch in range(2):
        FusedMLPPartner.launch([p.plain for p in ps], [p.rows for p in ps], ts)
        _launch_ac(ps, ts, F, C, odt, n)
        for k, p in enumerate(ps):
            tag = "F%d C%d %s n%d x%d player %d launch %d" % (F, C, odt, n, scale, k, launch)
            p.guards_intact()
            pairs = p.pairs[:2 * n].view(n, 2)
            assert torch.equal(pairs, p.plain.pairs), tag
            assert torch.equal(_bits(p.logits[:(4 + C) * n].view(4 + C, n)), _bits(p.plain.logits)), tag
            assert torch.equal(p.rng[:2 * n].view(2, n), p.plain._rng), tag
            assert torch.equal(p.move[:n], pairs[:, 0]) and torch.equal(p.comm[:n], pairs[:, 1]), tag
            mutants = n >= 33
            _check_value(p, p.value[:n].cpu().numpy().astype(np.float64), tsn, tag, mutants)
            _check_log_prob(p, p.log_prob[:n].cpu().numpy().astype(np.float64), pairs.cpu().numpy(), tsn, tag, mutants)


@pytest.mark.parametrize("F,C,odt,n,scale", [(29, 2, "float32", 33, 4), (35, 5, "int8", 97, 1)],
                         ids=["F29-C2-float32-n33", "F35-C5-int8-n97"])
def test_given_actions_are_scored_and_the_streams_stay(F, C, odt, n, scale):
    p = Player(F, C, odt, n, 40 + F, scale, True, 5)
    ts = torch.from_numpy(ar.make_timesteps(n, 500, 3)).cuda()
    tsn = ts.cpu().numpy()
    rng0 = p.rng.clone()
    p.ac._buffers(n)
    own0 = p.ac._rng.clone()
    obs = SimpleNamespace(rows=p.rows, timestep=ts)
    sums, sum_bound = np.zeros((2, n)), np.zeros((2, n))
    one = np.zeros((n, 2), np.int64)
    for mv in range(4):
        for cm in range(C):
            acts = np.tile(np.array([[mv, cm]], np.int32), (n, 1))
            given = torch.from_numpy(acts).cuda()
            _launch_ac([p], ts, F, C, odt, n, given=given, pairs=(mv + cm) % 2 == 0)
            p.guards_intact()
            assert torch.equal(p.rng, rng0)                       # neither read nor advanced
            assert (p.move[:n] == mv).all() and (p.comm[:n] == cm).all()
            got = p.log_prob[:n].cpu().numpy().astype(np.float64)
            _check_log_prob(p, got, acts, tsn, "given (%d, %d)" % (mv, cm), False)
            _check_value(p, p.value[:n].cpu().numpy().astype(np.float64), tsn, "given (%d, %d)" % (mv, cm), False)
            # the partner's score() is that launch
            lp, val = p.ac.score(obs, given)
            assert torch.equal(_bits(lp), _bits(p.log_prob[:n])) and torch.equal(_bits(val), _bits(p.value[:n]))
    # per head, the probabilities sum to 1 within the summed bounds: fix the other head at action 0
    # and subtract its (reference) term -- its own error is inside the bound of every launch
    for head, count in ((0, 4), (1, C)):
        total, tb = np.zeros(n), np.zeros(n)
        for a in range(count):
            acts = one.copy()
            acts[:, head] = a
            given = torch.from_numpy(acts.astype(np.int32)).cuda()
            lp, _ = p.ac.score(obs, given)
            _, terms = ar.ref_log_prob(p.w, p.rows_np, tsn, acts)
            total += np.exp(lp.cpu().numpy().astype(np.float64) - terms[1 - head])
            tb += np.exp(terms[head]) * np.expm1(ar.log_prob_bound(p.w, p.rows_np, tsn, acts))
        assert (np.abs(total - 1) <= tb + 1e-12).all(), (head, np.abs(total - 1).max(), tb.min())
    assert torch.equal(p.ac._rng, own0) and torch.equal(p.rng, rng0)
    # an index outside its head's range: -inf for that env only, everything else as before
    acts = np.tile(np.array([[1, C - 1]], np.int32), (n, 1))
    good = torch.from_numpy(acts).cuda()
    lp0, v0 = p.ac.score(obs, good)
    acts[0, 0], acts[n // 2, 1], acts[n - 1, 1] = 4, C, -1
    lp1, v1 = p.ac.score(obs, torch.from_numpy(acts).cuda())
    hit = [0, n // 2, n - 1]
    assert torch.isneginf(lp1[hit]).all()
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[hit] = False
    assert torch.equal(_bits(lp1[rest]), _bits(lp0[rest])) and torch.equal(_bits(v1), _bits(v0))
    # the raw launch echoes the index it was given into pairs and the action rows (include/oc_policy.h),
    # in range or not; the streams stay, and so does everything behind n
    bad = torch.from_numpy(acts).cuda()
    _launch_ac([p], ts, F, C, odt, n, given=bad)
    p.guards_intact()
    assert torch.equal(p.pairs[:2 * n].view(n, 2), bad)
    assert torch.equal(p.move[:n], bad[:, 0]) and torch.equal(p.comm[:n], bad[:, 1])
    assert torch.equal(_bits(p.log_prob[:n]), _bits(lp1)) and torch.equal(_bits(p.value[:n]), _bits(v1))
    assert torch.equal(p.rng, rng0) and torch.equal(p.ac._rng, own0)


def test_scoring_a_batch_of_another_size_leaves_the_seat_as_it_is():
    """A learner scores minibatches of recorded rows: their n is not the seat's.  ``score`` then
    equals a raw launch on that batch, and the seat's own tensors -- whose addresses a captured
    closed loop holds -- are neither reallocated nor changed."""
    from gym_comm_amd.vec_env import FusedActorCriticPartner
    F, C, odt, n_seat, n = 29, 2, "float32", 97, 33
    p = Player(F, C, odt, n, 40 + F, 4, True, 5)
    ts = torch.from_numpy(ar.make_timesteps(n, 500, 3)).cuda()
    given = torch.from_numpy(np.random.default_rng(2).integers(0, (4, C), (n, 2)).astype(np.int32)).cuda()
    batch = SimpleNamespace(rows=p.rows, timestep=ts)
    _launch_ac([p], ts, F, C, odt, n, given=given)
    want_lp, want_v = p.log_prob[:n].clone(), p.value[:n].clone()

    # a seat that has never acted owns nothing, before and after
    fresh = FusedActorCriticPartner(p.pol, sample=True, seed=8)
    lp, val = fresh.score(batch, given)
    assert torch.equal(_bits(lp), _bits(want_lp)) and torch.equal(_bits(val), _bits(want_v))
    assert fresh._rng is None and fresh.episode_start is None and fresh.log_prob is None and fresh.value is None

    # a seat in the middle of a rollout of n_seat envs
    seat = FusedActorCriticPartner(p.pol, sample=True, seed=8, keep_logits=True)
    own = SimpleNamespace(rows=torch.from_numpy(ar.make_rows(F, n_seat, odt, 77)).cuda(),
                          timestep=torch.from_numpy(ar.make_timesteps(n_seat, 500, 4)).cuda())
    act = torch.zeros((2, n_seat), dtype=torch.int32, device="cuda")
    seat.act_into(own, act[0], act[1])
    seat.update(torch.zeros(n_seat, device="cuda"), torch.arange(n_seat, device="cuda") % 3 == 0)
    held = [seat._rng, seat.episode_start, seat.log_prob, seat.value, seat.logits]
    before = [(t.data_ptr(), t.clone()) for t in held]
    assert 0 < int(seat.episode_start.sum().item()) < n_seat and not (seat._rng == pcg_fresh(seat, n_seat)).all()
    lp, val = seat.score(batch, given)
    torch.cuda.synchronize()
    assert lp.shape == (n,) and val.shape == (n,)
    assert torch.equal(_bits(lp), _bits(want_lp)) and torch.equal(_bits(val), _bits(want_v))
    now = [seat._rng, seat.episode_start, seat.log_prob, seat.value, seat.logits]
    for t, (ptr, was) in zip(now, before):
        assert t.data_ptr() == ptr and t.shape == was.shape and torch.equal(_bits(t), _bits(was))
    # and the seat goes on from where it was: the next act_into draws what an undisturbed twin draws
    twin = FusedActorCriticPartner(p.pol, sample=True, seed=8)
    act2 = torch.zeros((2, n_seat), dtype=torch.int32, device="cuda")
    twin.act_into(own, act2[0], act2[1])
    twin.act_into(own, act2[0], act2[1])
    seat.act_into(own, act[0], act[1])
    assert torch.equal(act, act2) and torch.equal(seat._rng, twin._rng)
    assert torch.equal(_bits(seat.log_prob), _bits(twin.log_prob))


def pcg_fresh(seat, n):
    from gym_comm_amd.batched import pcg32_seed_states
    return pcg32_seed_states(seat.seed, (2, n), seat.device)


# ---- the seat -----------------------------------------------------------------------------------
SC, ST, SN, TMAX = 2, 16, 64, 7


def _seat(graph):
    from gym_comm_amd.vec_env import (FusedActorCriticPartner, MLPActorCritic, OvercookedVecEnv, RandomPartner,
                                      RolloutSink)
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=TMAX, ego_config={},
                          partner_config={}, num_communication=SC, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, SN, seed=5, obs_dtype=torch.float32)
    F = 22 + venv._b.S + 2 * SC
    pol = MLPActorCritic(venv._b.S, SC, seed=31)
    with torch.no_grad():
        for t in pol.parameters():
            t.mul_(4)
    pol = pol.cuda()
    sink = RolloutSink(ST, SN, F, obs_dtype=torch.float32, fused=True)
    venv.partner = seat = FusedActorCriticPartner(pol, sample=True, seed=12, sink=sink)
    ego = RandomPartner(SC, seed=9)              # a seeded random ego, written into ego_action_rows
    venv.reset_tensors()
    loop = venv.closed_loop(ego, graph=graph, steps=ST if graph else 1)
    return SimpleNamespace(venv=venv, pol=pol, sink=sink, seat=seat, ego=ego, loop=loop, F=F)


def _sink_tensors(s):
    return [s.obs, s.timestep, s.actions, s.log_probs, s.values, s.rewards, s.episode_starts, s.dones, s.pos,
            s.last, s.count]


def test_the_learner_seat_records_through_the_fused_sink_eager_and_captured():
    e = _seat(False)
    rew, done = [], []
    for k in range(ST):
        _, r, d = e.loop.step()
        rew.append(r.clone())
        done.append(d.clone())
    rew, done = torch.stack(rew), torch.stack(done)
    s = e.sink
    assert s.steps() == ST and s.full()
    assert int(done.sum().item()) >= SN                              # every env finished an episode
    assert torch.equal(_bits(s.rewards), _bits(rew)) and torch.equal(s.dones, done)
    es = torch.cat([torch.ones((1, SN), device="cuda"), done[:-1].float()])
    assert torch.equal(s.episode_starts, es)
    assert torch.equal(e.seat.episode_start, done[-1].float())
    assert torch.equal(s.actions[-1, 0], e.venv._act[2]) and torch.equal(s.actions[-1, 1], e.venv._act[3])
    # every slot's log_prob and value from the recorded rows, timestep and actions
    w, wv, bv = ar.weights(e.pol)
    p = SimpleNamespace(w=w, wv=wv, bv=bv, n=SN, C=SC)
    for k in range(ST):
        p.rows_np = s.obs[k].cpu().numpy()
        tsn = s.timestep[k].cpu().numpy()
        _check_value(p, s.values[k].cpu().numpy().astype(np.float64), tsn, "seat slot %d" % k, True)
        _check_log_prob(p, s.log_probs[k].cpu().numpy().astype(np.float64), s.actions[k].T.cpu().numpy(), tsn,
                        "seat slot %d" % k, True)
    assert torch.equal(_bits(s.log_probs[-1]), _bits(e.seat.log_prob)) and torch.equal(_bits(s.values[-1]), _bits(e.seat.value))
    # returns and advantages: the float32 loop on the recorded rows, bit for bit
    adv, ret = e.seat.finish_rollout()
    ea, er = rollout_ref.gae(s.rewards.cpu().numpy(), s.values.cpu().numpy(), s.episode_starts.cpu().numpy(),
                             e.seat.value.cpu().numpy(), e.seat.episode_start.cpu().numpy(), 0.99, 0.95, np.float32)
    assert np.array_equal(adv.cpu().numpy().view(np.int32), ea.view(np.int32))
    assert np.array_equal(ret.cpu().numpy().view(np.int32), er.view(np.int32))
    assert s.steps() == ST

    # the same run as ONE captured 16-step closed loop
    g = _seat(True)
    g.loop.step()
    torch.cuda.synchronize()
    for a, b in zip(_sink_tensors(g.sink), _sink_tensors(s)):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(g.seat.get_state(SN)[:4] + (g.ego.get_state(SN),), e.seat.get_state(SN)[:4] + (e.ego.get_state(SN),)):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(g.venv._b._arena, e.venv._b._arena) and torch.equal(g.venv._act, e.venv._act)

    # get_state / set_state: restoring and repeating 4 steps reproduces the same 4 slots
    b = e.venv._b
    saved = (e.seat.get_state(SN), e.ego.get_state(SN), b._arena.clone(), e.venv._act.clone(),
             None if b.rng is None else b.rng.clone())
    slots = []
    for rep in range(2):
        for _ in range(4):
            e.loop.step()
        slots.append([t.clone() for t in _sink_tensors(s)] + [e.seat._rng.clone(), e.seat.episode_start.clone()])
        if rep == 0:
            assert int(s.pos.item()) == 4 and s.steps() == ST + 4
            assert not torch.equal(e.seat._rng, saved[0][0])
            e.seat.set_state(saved[0])
            e.ego.set_state(saved[1])
            b._arena.copy_(saved[2])
            e.venv._act.copy_(saved[3])
            if saved[4] is not None:
                b.rng.copy_(saved[4])
            assert int(s.pos.item()) == 0 and s.steps() == ST
    for a, c in zip(*slots):
        assert torch.equal(_bits(a), _bits(c))
