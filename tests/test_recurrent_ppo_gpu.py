"""-m gpu: the recurrent PPO update (include/oc_policy.h, last section: oc_policy_rppo_update / _grad;
``RecurrentPPOLearner``) against the float64 reference of tests/recurrent_ppo_ref.py, on the smallest cases at
which each mechanism can fail:

    a   T = 1, n = 32, envs [5, 5]          F 14, C 1, int8      no recurrence; E T = 2, the smallest; a repeated env;
                                                                 one x k-step
    b   T = 2, n = 40, 33 envs, permuted    F 29, C 5, int32     one carry; a full tile + 1 lane; two x k-steps
    c   T = 7, n = 100, 96 envs, permuted,  F 62, C 16, float32  three tiles; four x k-steps; starts at t = 0, 3, 6;
        one repeat                                               weights x 2

and on tests/recurrent_ppo_ref.py's ``edge_cases`` d, e, e48, f, g: the paths a full-size minibatch takes -- a ragged
last round of the weight-gradient kernel, int8 rows beyond t = 0, F + 2 = 17, 32, 33, 48, 49, 52 steps, E = 1 and 32.
"""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import recurrent_ppo_ref as rp  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}
_CASES = {}
ALL = ["a", "b", "c", "d", "e", "e48", "f", "g"]


def _case(name):
    """The shared cases and their references, built once (a family at its first use) and never changed."""
    if name not in _CASES:
        hp = rp.test_hp()
        for k, c in (rp.gpu_cases() if name in "abc" else rp.edge_cases()):
            _CASES[k] = (c, rp.loss_and_grad(c, hp, emulate=True))
    return _CASES[name]


def _setup(case, hp=None, max_groups=0):
    from gym_comm_amd.vec_env import FusedRecurrentPartner, RecurrentPPOLearner, RolloutSink
    hp = hp or rp.test_hp()
    T, F, n = case["obs"].shape
    pol = copy.deepcopy(case["pol"]).float().cuda()
    seat = FusedRecurrentPartner(pol, sample=True, seed=5)
    sink = RolloutSink(T, n, F, obs_dtype=DT[case["odt"]], fused=True)
    put = lambda t, a: t.copy_(torch.from_numpy(np.ascontiguousarray(a)))  # noqa: E731
    put(sink.obs, case["obs"]), put(sink.timestep, case["ts"]), put(sink.actions, case["actions"])
    put(sink.log_probs, case["old_lp"]), put(sink.advantages, case["adv"]), put(sink.returns, case["ret"])
    put(sink.episode_starts, case["es"])
    sink.count.fill_(T)                                  # a full sink in chronological order: pos stays 0
    sink.returns_ready = True
    seat.begin_rollout(n)
    put(seat.h0, case["h0"]), put(seat.c0, case["c0"])
    learner = RecurrentPPOLearner(seat, lr=hp.lr, clip_range=hp.clip, ent_coef=hp.ent, vf_coef=hp.vf,
                                  max_grad_norm=hp.max_norm, betas=(hp.b1, hp.b2), eps=hp.eps, max_groups=max_groups)
    envs = torch.from_numpy(np.asarray(case["envs"], np.int32)).cuda()
    return SimpleNamespace(case=case, hp=hp, pol=pol, seat=seat, sink=sink, learner=learner, envs=envs, T=T, n=n, F=F,
                           E=envs.numel())


def _grads(e):
    e.learner.grad(e.sink, e.envs)
    torch.cuda.synchronize()
    return ({k: v.detach().cpu().numpy().astype(np.float64) for k, v in e.learner.grads.items()}, e.learner.stats())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.float16 else t


@pytest.mark.parametrize("name", ALL)
def test_the_forward_is_T_chained_scoring_launches_bit_for_bit(name):
    case, _ = _case(name)
    e = _setup(case)
    lp_out, v_out = torch.full((e.T, e.E), 7.0, device="cuda"), torch.full((e.T, e.E), 7.0, device="cuda")
    e.learner.lp_out, e.learner.v_out = lp_out, v_out
    e.learner.grad(e.sink, e.envs)
    ix = e.envs.long()
    h, c = e.seat.h0[:, ix].contiguous(), e.seat.c0[:, ix].contiguous()
    for t in range(e.T):
        rows, ts = e.sink.obs[t][:, ix].contiguous(), e.sink.timestep[t][ix].contiguous()
        es, pairs = e.sink.episode_starts[t][ix].contiguous(), e.sink.actions[t][:, ix].T.contiguous()
        lp, val = torch.empty(e.E, device="cuda"), torch.empty(e.E, device="cuda")
        h2, c2 = torch.empty_like(h), torch.empty_like(c)
        e.seat._launch(rows, ts, (h, c), (h2, c2), es, pairs, None, None, lp, val)     # score(), keeping the new state
        assert torch.equal(_bits(lp_out[t]), _bits(lp)) and torch.equal(_bits(v_out[t]), _bits(val)), t
        h, c = h2, c2
    assert torch.isfinite(lp_out).all()


@pytest.mark.parametrize("name", ALL)
def test_the_gradient_and_the_statistics_against_the_reference_and_every_mutant_is_rejected(name):
    case, (ref, stats, inter) = _case(name)
    tol_g, tol_s = rp.tolerances(name)
    e = _setup(case)
    got, gstats = _grads(e)
    d = rp.rel_diff(got, ref)
    sd = rp.stats_diff(gstats, stats)
    print("case", name, "grad", {k: "%.3g" % v for k, v in d.items()}, "largest %.3g" % max(d.values()))
    print("case", name, "stats", {k: "%.3g" % v for k, v in sd.items()}, "largest %.3g" % max(sd.values()))
    assert max(d.values()) <= tol_g, d
    assert max(sd.values()) <= tol_s, sd
    if name == "g":
        # one sequence does not separate every planted bug by twenty tolerances: the tolerance alone, and no
        # tensor's gradient may be missing
        assert all(np.abs(got[k]).max() > 0 for k in rp.NAMES), {k: np.abs(got[k]).max() for k in rp.NAMES}
        return
    for m in rp.MUTANTS:
        mref = rp.loss_and_grad(case, e.hp, emulate=True, mutate=m, steps=inter["steps"])[0]
        if max(rp.rel_diff(mref, ref).values()) == 0:
            assert name in "abc", (name, m)              # every mutant applies to d, e, e48 and f
            continue                                     # the mutant does not apply to this case (tests/test_recurrent_ppo_cpu.py)
        assert max(rp.rel_diff(got, mref).values()) > tol_g, m


def test_a_starting_envs_old_state_reaches_nothing():
    case, _ = _case("c")
    e = _setup(case)
    env = int(case["envs"][0])
    assert case["es"][0, env] == 1.0
    lp, v = torch.zeros((e.T, e.E), device="cuda"), torch.zeros((e.T, e.E), device="cuda")
    e.learner.lp_out, e.learner.v_out = lp, v
    want, wstats = _grads(e)
    wlp, wv = lp.clone(), v.clone()
    e.seat.h0[3, env], e.seat.c0[60, env] = float("nan"), float("inf")
    got, gstats = _grads(e)
    assert all(np.isfinite(g).all() for g in got.values()) and all(np.isfinite(x) for x in gstats.values())
    assert all(np.array_equal(got[k], want[k]) for k in got) and gstats == wstats
    assert torch.equal(_bits(lp), _bits(wlp)) and torch.equal(_bits(v), _bits(wv))


def test_a_bad_action_is_counted_and_contributes_nothing():
    base, _ = _case("b")
    case = copy.deepcopy(base)
    env = int(case["envs"][7])
    case["actions"][0, 1, env] = 4 + case["C"]           # step 0, comm head: out of range
    ref, stats, it = rp.loss_and_grad(case, rp.test_hp(), emulate=True)
    assert stats["bad"] == 1.0 and not it["good"][7]
    e = _setup(case)
    lp = torch.zeros((e.T, e.E), device="cuda")
    e.learner.lp_out = lp
    got, gstats = _grads(e)
    assert gstats["bad"] == 1.0 and lp[0, 7].item() == float("-inf") and torch.isfinite(lp[1]).all()
    d, sd = rp.rel_diff(got, ref), rp.stats_diff(gstats, stats)
    assert max(d.values()) <= rp.TOL_G and max(sd.values()) <= rp.TOL_S, (d, sd)
    # ... and differs from the gradient with that sample in
    assert max(rp.rel_diff(got, _case("b")[1][0]).values()) > rp.TOL_G


def test_the_same_call_gives_the_same_bits_and_one_workgroup_agrees():
    case, (ref, stats, _) = _case("c")
    e = _setup(case)
    g1, s1 = _grads(e)
    g2, s2 = _grads(e)
    assert all(np.array_equal(g1[k], g2[k]) for k in g1) and s1 == s2
    assert e.learner.plan(e.E, e.T)[1] == 21
    one = _setup(case, max_groups=1)
    assert one.learner.plan(one.E, one.T)[1:3] == (1, 21)
    g3, s3 = _grads(one)
    d, sd = rp.rel_diff(g3, ref), rp.stats_diff(s3, stats)
    print("max_groups 1:", {k: "%.3g" % v for k, v in d.items()})
    assert max(d.values()) <= rp.TOL_G and max(sd.values()) <= rp.TOL_S
    assert max(rp.rel_diff(g3, g1).values()) <= rp.TOL_G


_ONE_GROUP = {}


@pytest.mark.parametrize("name,max_groups,groups,per", [("c", 4, 4, 6), ("d", 0, 256, 2), ("d", 7, 7, 38)])
def test_a_ragged_last_round_of_the_weight_gradient(name, max_groups, groups, per):
    """Gw does not divide the T ceil(E / 32) items: in the last round the workgroups past the end skip the item, and
    both of its barriers.  c, 4: 21 items in 24 slots; d, default cap: 260 in 512, the second round 4 live of 256;
    d, 7: 260 in 266."""
    case, (ref, stats, _) = _case(name)
    tol_g, tol_s = rp.tolerances(name)
    e = _setup(case, max_groups=max_groups)
    tiles, Gw, rounds = e.learner.plan(e.E, e.T)[:3]
    assert (Gw, rounds) == (groups, per) and Gw * rounds > tiles * e.T > Gw * (rounds - 1)
    g1, s1 = _grads(e)
    g2, s2 = _grads(e)
    assert all(np.array_equal(g1[k], g2[k]) for k in g1) and s1 == s2
    d, sd = rp.rel_diff(g1, ref), rp.stats_diff(s1, stats)
    print("case", name, "max_groups", max_groups, "(Gw, per)", (Gw, rounds), "grad", {k: "%.3g" % v for k, v in d.items()},
          "largest %.3g" % max(d.values()), "stats largest %.3g" % max(sd.values()))
    assert max(d.values()) <= tol_g, d
    assert max(sd.values()) <= tol_s, sd
    if name not in _ONE_GROUP:
        one = _setup(case, max_groups=1)
        assert one.learner.plan(one.E, one.T)[1:3] == (1, tiles * e.T)
        _ONE_GROUP[name] = _grads(one)[0]
        d1 = rp.rel_diff(_ONE_GROUP[name], ref)
        print("case", name, "max_groups 1: grad", {k: "%.3g" % v for k, v in d1.items()}, "largest %.3g" % max(d1.values()))
        assert max(d1.values()) <= tol_g, d1
    dd = rp.rel_diff(g1, _ONE_GROUP[name])
    print("against max_groups 1:", {k: "%.3g" % v for k, v in dd.items()})
    assert max(dd.values()) <= tol_g, dd


def _images(e):
    return [t.clone() for t in e.seat._w] + [e.learner._bwd.clone()]


def test_three_updates_are_adam_on_the_kernels_own_gradient_and_repack_the_images():
    _updates_are_adam_and_repack("c", 3)


@pytest.mark.parametrize("name", ["d", "e"])
def test_an_update_of_an_edge_case_is_adam_and_repacks_the_images(name):
    """d: the clip, Adam and the repack behind 52 steps' gradient, int8 rows and the default (ragged) plan; F + 2 = 32,
    the timestep and the bias column are the last two of the second x k-step and the repack's ``k >= F + 2`` arm is
    never taken.  e: F + 2 = 33, the third k-step holds the bias column and fifteen columns of that arm's zeros."""
    _updates_are_adam_and_repack(name, 1)


def _updates_are_adam_and_repack(name, updates):
    from gym_comm_amd.partners import pack_lstm, pack_lstm_bwd
    case, _ = _case(name)
    hp = rp.test_hp(max_grad_norm=0.05)                  # an active clip
    e = _setup(case, hp=hp)
    L = e.learner
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64).reshape(-1)  # noqa: E731
    flat = lambda: np.concatenate([f64(getattr(e.pol, k)) for k in rp.NAMES])  # noqa: E731
    for step in range(1, updates + 1):
        w, m, v = flat(), f64(L.m), f64(L.v)
        L.update(e.sink, e.envs)
        torch.cuda.synchronize()
        g = f64(L.grad_flat)                             # the clipped gradient the update applied
        assert L.stats()["grad_norm"] > hp.max_norm and abs(np.sqrt((g ** 2).sum()) - hp.max_norm) < 1e-4 * hp.max_norm
        w2, m2, v2 = rp.adam(w, m, v, g, step, hp)
        ew, em, ev = rp.adam_bound(w, m, v, g, step, hp)
        assert (np.abs(flat() - w2) <= ew).all() and (np.abs(f64(L.m) - m2) <= em).all() and (np.abs(f64(L.v) - v2) <= ev).all()
        assert not np.array_equal(flat(), w) and int(L.step.item()) == step
        want = pack_lstm(L._L, e.pol)
        for have, arr in zip(e.seat._w, want):
            host = torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr)
            assert torch.equal(_bits(have.cpu()).reshape(-1), _bits(host).reshape(-1))
        assert torch.equal(_bits(L._bwd.cpu()), _bits(torch.from_numpy(pack_lstm_bwd(L._L, e.pol))))


def _state(e):
    return [t.detach().clone() for t in list(e.pol.parameters()) + [e.learner.m, e.learner.v, e.learner.step,
                                                                      e.learner.grad_flat, e.learner.stats_t]] + _images(e)


def _restore(e, saved):
    live = list(e.pol.parameters()) + [e.learner.m, e.learner.v, e.learner.step, e.learner.grad_flat, e.learner.stats_t] \
        + list(e.seat._w) + [e.learner._bwd]
    with torch.no_grad():
        for t, s in zip(live, saved):
            t.copy_(s)


def test_a_captured_update_replays_with_rewritten_envs():
    case, _ = _case("b")
    rng = np.random.default_rng(5)
    e1 = torch.from_numpy(rng.permutation(40)[:33].astype(np.int32)).cuda()
    e2 = torch.from_numpy(rng.integers(0, 40, 33).astype(np.int32)).cuda()
    a = _setup(case)
    a.learner.update(a.sink, e1)
    a.learner.update(a.sink, e2)
    torch.cuda.synchronize()
    want = _state(a)
    b = _setup(case)
    start = _state(b)
    buf = e1.clone()
    b.learner.update(b.sink, buf)                        # every kernel has run once before the capture
    torch.cuda.synchronize()
    _restore(b, start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.learner.update(b.sink, buf)
    _restore(b, start)                                   # whether or not the capture ran anything
    graph.replay()
    buf.copy_(e2)
    graph.replay()
    torch.cuda.synchronize()
    assert int(b.learner.step.item()) == 2
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(want, _state(b)))


def test_train_on_a_rollout_collected_by_the_closed_loop():
    from gym_comm_amd.vec_env import (FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RandomPartner,
                                      RecurrentPPOLearner, RolloutSink)
    SC, ST, SN = 2, 8, 64
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=7, ego_config={},
                          partner_config={}, num_communication=SC, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, SN, seed=5, obs_dtype=torch.float32)
    F = 22 + venv._b.S + 2 * SC
    pol = LSTMActorCritic(venv._b.S, SC, seed=31).cuda()
    sink = RolloutSink(ST, SN, F, obs_dtype=torch.float32, fused=True)
    venv.partner = seat = FusedRecurrentPartner(pol, sample=True, seed=12, sink=sink)
    venv.reset_tensors()
    loop = venv.closed_loop(RandomPartner(SC, seed=9), graph=False, steps=1)
    # vf_coef: the cell is shared by actor and critic, and on a fresh module the value loss (returns near -20
    # against values near 0) is four hundred times the policy term: at vf_coef 0.5 the clipped step is the
    # critic's, and which way it drags the log-probs says nothing about the policy gradient this test is about
    learner = RecurrentPPOLearner(seat, lr=1e-3, ent_coef=0.0, vf_coef=1e-3)
    for _ in range(3):                                   # a rollout before this one: the start state is not zero
        loop.step()
    seat.begin_rollout()
    assert sink.steps() == 0 and seat.h0.abs().sum() > 0 and torch.equal(seat.h0, seat.h)
    with pytest.raises(ValueError):                      # nothing recorded, no advantages
        learner.train(sink, n_epochs=1)
    for _ in range(ST - 1):
        loop.step()
    seat.finish_rollout()
    with pytest.raises(ValueError, match="full"):        # advantages, but one step short
        learner.train(sink, n_epochs=1)
    loop.step()
    with pytest.raises(ValueError):                      # a plain sink has no advantages
        learner.train(RolloutSink(ST, SN, F, obs_dtype=torch.float32), n_epochs=1)
    seat.finish_rollout()
    assert sink.episode_starts.sum() > 0                 # max_num_timesteps 7: episodes end inside the rollout
    batches = learner.minibatches(sink, 32, generator=torch.Generator(device="cuda").manual_seed(3))
    assert [b.numel() for b in batches] == [32, 32] and batches[0].dtype == torch.int32
    assert torch.equal(torch.cat(batches).sort().values.cpu(), torch.arange(SN, dtype=torch.int32))
    everyone = torch.arange(SN, dtype=torch.int32, device="cuda")
    lp0 = torch.zeros((ST, SN), device="cuda")
    learner.lp_out = lp0
    learner.grad(sink, everyone)
    assert (lp0 - sink.log_probs).abs().max() < 1e-5     # the unrolled forward finds the recorded log-probs again
    learner.lp_out = None
    before = [t.detach().clone() for t in pol.parameters()]
    learner.train(sink, n_epochs=4)
    stats = learner.stats()
    print("train():", stats)
    assert int(learner.step.item()) == 4 and stats["bad"] == 0.0
    assert all(torch.isfinite(t).all() for t in pol.parameters()) and all(np.isfinite(v) for v in stats.values())
    assert all(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    lp1 = torch.zeros((ST, SN), device="cuda")
    learner.lp_out = lp1
    learner.grad(sink, everyone)
    adv = sink.advantages.double()
    up = (adv - adv.mean()) / (adv.std() + 1e-8) > 0
    rose = (lp1 - lp0)[up].double().mean().item()
    print("mean log-prob change where A^ > 0: %.5f" % rose)
    assert rose > 0
    loop.step()                                          # the seat acts afterwards, on the new weights
    assert torch.isfinite(seat.log_prob).all() and torch.isfinite(seat.value).all()


def test_train_refuses_a_sink_out_of_chronological_order():
    case, _ = _case("b")
    e = _setup(case)
    e.learner.train(e.sink, n_epochs=1, granule=1)       # as set up: full, advantages, pos 0
    e.sink.pos.fill_(1)
    with pytest.raises(ValueError, match="chronological"):
        e.learner.train(e.sink, n_epochs=1, granule=1)
    e.sink.pos.fill_(0)
    e.sink.count.fill_(e.T + 1)                          # the ring has wrapped
    with pytest.raises(ValueError, match="chronological"):
        e.learner.train(e.sink, n_epochs=1, granule=1)
    e.sink.count.fill_(e.T - 1)
    with pytest.raises(ValueError, match="full"):
        e.learner.train(e.sink, n_epochs=1, granule=1)
    e.sink.count.fill_(e.T)
    e.sink.returns_ready = False
    with pytest.raises(ValueError, match="advantages"):
        e.learner.train(e.sink, n_epochs=1, granule=1)
    with pytest.raises(TypeError):
        from gym_comm_amd.vec_env import FusedActorCriticPartner, MLPActorCritic, RecurrentPPOLearner
        RecurrentPPOLearner(FusedActorCriticPartner(MLPActorCritic(3, 2).cuda()))
