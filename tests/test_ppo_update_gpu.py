"""GPU: the PPO update of the fused actor-critic seat (include/oc_policy.h: oc_policy_ppo_update / oc_policy_ppo_grad,
gym_comm_amd.vec_env.PPOLearner) against the float64 reference and the derived bounds of
tests/ppo_ref.py, on a synthetic rollout of T = 3 slots x n = 70 envs (210 samples, no multiple of 32).
Every figure is printed before it is asserted."""
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
import ppo_ref as pp  # noqa: E402

pytestmark = pytest.mark.gpu
TORCH_DT = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _setup(F, C, odt, scale, seed, hp=None, max_groups=0):
    """A buffer of ppo_ref.make_buffer in a fused RolloutSink, the module on the GPU in a seat, the
    recorded log-probs and values from score() under the `old` module, and a learner."""
    from gym_comm_amd.vec_env import FusedActorCriticPartner, PPOLearner, RolloutSink
    hp = hp or pp.test_hp()
    buf = pp.make_buffer(F, C, odt, scale, seed)
    T, n = pp.T_SLOTS, pp.N_ENVS
    sink = RolloutSink(T, n, F, obs_dtype=TORCH_DT[odt], fused=True)
    sink.obs.copy_(torch.from_numpy(buf["obs"]))
    sink.timestep.copy_(torch.from_numpy(buf["ts"]))
    sink.actions.copy_(torch.from_numpy(buf["actions"]))
    sink.advantages.copy_(torch.from_numpy(buf["adv"]))
    sink.returns.copy_(torch.from_numpy(buf["ret"]))
    old = FusedActorCriticPartner(buf["old"].cuda(), sample=False)
    for s in range(T):
        lp, v = old.score(SimpleNamespace(rows=sink.obs[s], timestep=sink.timestep[s]), sink.actions[s].T.contiguous())
        sink.log_probs[s].copy_(lp)
        sink.values[s].copy_(v)
    pol = copy.deepcopy(buf["pol"]).cuda()
    seat = FusedActorCriticPartner(pol, sample=False)
    learner = PPOLearner(seat, lr=hp.lr, clip_range=hp.clip, ent_coef=hp.ent, vf_coef=hp.vf,
                         max_grad_norm=hp.max_norm, betas=(hp.b1, hp.b2), eps=hp.eps, max_groups=max_groups)
    return SimpleNamespace(buf=buf, sink=sink, pol=pol, seat=seat, learner=learner, hp=hp,
                           old_lp=sink.log_probs.cpu().numpy())


def _gathered_score(e, idx):
    """score() of the samples `idx`, gathered by torch."""
    n = pp.N_ENVS
    i = idx.long()
    slot, env = i // n, i % n
    rows = e.sink.obs[slot, :, env].T.contiguous()
    ts = e.sink.timestep.reshape(-1)[i].contiguous()
    pairs = e.sink.actions[slot, :, env].contiguous()
    return e.seat.score(SimpleNamespace(rows=rows, timestep=ts), pairs)


_runs = {}


def _grad_run(case):
    """One oc_policy_ppo_grad per case, shared by the forward and the gradient test."""
    if case not in _runs:
        F, C, odt, scale, B, mg, seed = case
        e = _setup(F, C, odt, scale, seed, max_groups=mg)
        idx_np = pp.make_indices(B)
        idx = torch.from_numpy(idx_np).cuda()
        e.learner.lp_out = torch.full((B,), 7.0, device="cuda")
        e.learner.v_out = torch.full((B,), 7.0, device="cuda")
        grads = e.learner.grad(e.sink, idx)
        torch.cuda.synchronize()
        e.idx, e.idx_np = idx, idx_np
        e.grads = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in grads.items()}
        e.stats = e.learner.stats()
        _runs[case] = e
    return _runs[case]


@pytest.mark.parametrize("case", pp.GRAD_CASES)
def test_forward_is_score_bit_for_bit(case):
    e = _grad_run(case)
    lp, v = _gathered_score(e, e.idx)
    assert torch.isfinite(lp).all()
    assert torch.equal(_bits(e.learner.lp_out), _bits(lp)) and torch.equal(_bits(e.learner.v_out), _bits(v))


@pytest.mark.parametrize("case", pp.GRAD_CASES)
def test_gradient_and_statistics_within_the_derived_bounds(case):
    e = _grad_run(case)
    F, C, odt, scale, B, mg, seed = case
    plan = e.learner.plan(B)
    assert plan[:2] == pp.ref_plan(B, mg)
    ref_case = pp.make_case(e.buf, e.idx_np, e.old_lp)
    bound, sb, ref, rstats = pp.grad_bound(ref_case, e.hp, plan)
    if B >= 210:                         # both clip sides occur, and some samples are inside
        _, _, it = pp.loss_and_grad(ref_case, e.hp)
        assert (it["ratio"] > 1 + e.hp.clip).any() and (it["ratio"] < 1 - e.hp.clip).any() and it["inside"].any()
    worst = pp.clipped_excess(e.grads, e.stats["grad_norm"], ref, bound, e.hp)
    excess = {k: v[0] for k, v in worst.items()}
    for k in pp.NAMES:
        print(case, k, "excess over the bound %.3e at kernel %.9e reference %.9e bound %.3e (largest bound %.3e, "
              "largest |g| %.3e)" % (worst[k] + (bound[k].max(), np.abs(ref[k]).max())))
    for k in pp.STATS:
        tol = sb[k] + 2 * pp.U * abs(rstats[k])
        print(case, k, "kernel %.9g reference %.9g bound %.3e" % (e.stats[k], rstats[k], tol))
    for k in pp.NAMES:
        assert excess[k] <= 0, (k, excess[k])
    for k in pp.STATS:
        assert abs(e.stats[k] - rstats[k]) <= sb[k] + 2 * pp.U * abs(rstats[k]), k


def test_a_bad_action_is_counted_and_contributes_nothing():
    F, C, odt, scale, B, mg, seed = pp.GRAD_CASES[0]
    e = _setup(F, C, odt, scale, seed, max_groups=mg)
    idx_np = pp.make_indices(B)
    s = int(idx_np[17])
    e.buf["actions"][s // pp.N_ENVS, 0, s % pp.N_ENVS] = 7             # a recorded move outside 0..3
    e.sink.actions.copy_(torch.from_numpy(e.buf["actions"]))
    grads = e.learner.grad(e.sink, torch.from_numpy(idx_np).cuda())
    stats = e.learner.stats()
    assert stats["bad"] == 1.0
    ref_case = pp.make_case(e.buf, idx_np, e.old_lp)
    bound, sb, ref, rstats = pp.grad_bound(ref_case, e.hp, e.learner.plan(B))
    assert rstats["bad"] == 1.0
    got = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in grads.items()}
    excess = pp.clipped_check(got, stats["grad_norm"], ref, bound, e.hp)
    print("bad action:", excess)
    assert all(np.isfinite(v).all() for v in got.values()) and max(excess.values()) <= 0
    for k in ("policy_loss", "value_loss", "entropy_loss", "loss"):
        assert abs(stats[k] - rstats[k]) <= sb[k] + 2 * pp.U * abs(rstats[k]), k


def _state(e):
    ln = e.learner
    return [t.detach().clone() for t in list(ln._params) + [ln.m, ln.v, ln.step, ln._w2t, ln.stats_t] + list(e.seat._w)]


def _restore(e, st):
    ln = e.learner
    with torch.no_grad():
        for t, s in zip(list(ln._params) + [ln.m, ln.v, ln.step, ln._w2t, ln.stats_t] + list(e.seat._w), st):
            t.copy_(s)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


APPLY = pp.GRAD_CASES[3]             # F = 46 (three k-steps), float32 rows, scale 4, one workgroup, two tiles per wave


def test_the_same_call_gives_the_same_bits():
    F, C, odt, scale, B, mg, seed = APPLY
    idx = torch.from_numpy(pp.make_indices(300)).cuda()
    out = []
    for _ in range(2):
        e = _setup(F, C, odt, scale, seed, max_groups=3)
        e.learner.grad(e.sink, idx)
        g = e.learner.grad_flat.clone()
        e.learner.grad(e.sink, idx)
        assert torch.equal(_bits(g), _bits(e.learner.grad_flat))
        e.learner.update(e.sink, idx)
        e.learner.update(e.sink, idx)
        out.append(_state(e) + [e.learner.grad_flat.clone()])
    torch.cuda.synchronize()
    assert _same_bits(out[0], out[1])


def test_three_updates_adam_and_the_repacked_fragments():
    from gym_comm_amd.vec_env import FusedActorCriticPartner, PPOLearner
    F, C, odt, scale, B, mg, seed = APPLY
    e = _setup(F, C, odt, scale, seed, max_groups=mg)
    ln, hp = e.learner, e.hp
    flat = lambda ts: np.concatenate([t.detach().cpu().numpy().astype(np.float64).reshape(-1) for t in ts])  # noqa: E731
    probe = torch.from_numpy(pp.make_indices(33)).cuda()
    for step in (1, 2, 3):
        idx = torch.from_numpy(pp.make_indices(B, seed=step)).cuda()
        w0, m0, v0 = flat(ln._params), flat([ln.m]), flat([ln.v])
        lp_before, _ = _gathered_score(e, probe)
        ln.update(e.sink, idx)
        g = flat([ln.grad_flat])
        w1, m1, v1 = flat(ln._params), flat([ln.m]), flat([ln.v])
        assert int(ln.step.item()) == step
        norm = ln.stats()["grad_norm"]
        assert norm > 2 * hp.max_norm                                 # the clip is active
        assert abs(np.sqrt((g ** 2).sum()) - hp.max_norm) <= 1e-5 * hp.max_norm
        rw, rm, rv = pp.adam(w0, m0, v0, g, step, hp)
        e_w, e_m, e_v = pp.adam_bound(w0, m0, v0, g, step, hp)
        for name, got, want, tol in (("w", w1, rw, e_w), ("m", m1, rm, e_m), ("v", v1, rv, e_v)):
            ex = (np.abs(got - want) - tol).max()
            print("step", step, name, "excess over the bound %.3e (largest bound %.3e, largest change %.3e)"
                  % (ex, tol.max(), np.abs(got - (w0 if name == "w" else 0)).max()))
            assert ex <= 0, (step, name, ex)
        assert np.abs(w1 - w0).max() > 0.5 * hp.lr
        # the fragments: bit for bit what the host packs from the same fp32 weights
        twin = FusedActorCriticPartner(copy.deepcopy(e.pol), sample=False)
        for k, (a, b) in enumerate(zip(e.seat._w, twin._w)):
            assert torch.equal(a, b), ("fragment", k, step)
        assert torch.equal(_bits(PPOLearner(twin)._w2t), _bits(ln._w2t))
        lp_after, v_after = _gathered_score(e, probe)
        lp_twin, v_twin = twin.score(*_probe_args(e, probe))
        assert torch.equal(_bits(lp_after), _bits(lp_twin)) and torch.equal(_bits(v_after), _bits(v_twin))
        assert not torch.equal(_bits(lp_after), _bits(lp_before))
    # an explicit refresh() repacks on the host, in place: the same address (captured graphs keep it)
    # and, from the weights the updates left, the same bits
    ptr, before = ln._w2t.data_ptr(), _bits(ln._w2t).clone()
    ln.refresh()
    assert ln._w2t.data_ptr() == ptr and torch.equal(_bits(ln._w2t), before)


def _probe_args(e, idx):
    n = pp.N_ENVS
    i = idx.long()
    slot, env = i // n, i % n
    return (SimpleNamespace(rows=e.sink.obs[slot, :, env].T.contiguous(),
                            timestep=e.sink.timestep.reshape(-1)[i].contiguous()),
            e.sink.actions[slot, :, env].contiguous())


def test_a_captured_update_replays_with_rewritten_indices():
    F, C, odt, scale, B, mg, seed = APPLY
    i1 = torch.from_numpy(pp.make_indices(B, seed=1)).cuda()
    i2 = torch.from_numpy(pp.make_indices(B, seed=2)).cuda()
    a = _setup(F, C, odt, scale, seed, max_groups=mg)
    a.learner.update(a.sink, i1)
    a.learner.update(a.sink, i2)
    want = _state(a)
    b = _setup(F, C, odt, scale, seed, max_groups=mg)
    start = _state(b)
    buf = i1.clone()
    b.learner.update(b.sink, buf)                    # every kernel has run once before the capture
    torch.cuda.synchronize()
    _restore(b, start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.learner.update(b.sink, buf)
    _restore(b, start)                               # whether or not the capture ran anything
    graph.replay()
    buf.copy_(i2)
    graph.replay()
    torch.cuda.synchronize()
    assert int(b.learner.step.item()) == 2
    assert _same_bits(want, _state(b))


def test_ten_updates_move_the_policy_the_way_the_advantages_point():
    hp = pp.HP(ent_coef=0.0, max_grad_norm=0.5, lr=3e-3)
    e = _setup(30, 3, "int8", 1, 33, hp=hp)
    idx_np = np.arange(pp.T_SLOTS * pp.N_ENVS, dtype=np.int32)
    idx = torch.from_numpy(idx_np).cuda()
    adv = e.buf["adv"].reshape(-1).astype(np.float64)
    ahat = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    up, down = torch.from_numpy(ahat > 0).cuda(), torch.from_numpy(ahat < 0).cuda()
    lp0, _ = _gathered_score(e, idx)
    for _ in range(10):
        e.learner.update(e.sink, idx)
    lp1, _ = _gathered_score(e, idx)
    rose, fell = (lp1 - lp0)[up].double().mean().item(), (lp1 - lp0)[down].double().mean().item()
    print("mean log-prob change: A^ > 0 %.4f, A^ < 0 %.4f" % (rose, fell))
    assert rose > 0 and fell < 0


def test_train_on_a_rollout_collected_by_the_closed_loop():
    from gym_comm_amd.vec_env import (FusedActorCriticPartner, MLPActorCritic, OvercookedVecEnv, PPOLearner,
                                      RandomPartner, RolloutSink)
    SC, ST, SN = 2, 8, 64
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=7, ego_config={},
                          partner_config={}, num_communication=SC, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, SN, seed=5, obs_dtype=torch.float32)
    F = 22 + venv._b.S + 2 * SC
    pol = MLPActorCritic(venv._b.S, SC, seed=31).cuda()
    sink = RolloutSink(ST, SN, F, obs_dtype=torch.float32, fused=True)
    venv.partner = seat = FusedActorCriticPartner(pol, sample=True, seed=12, sink=sink)
    venv.reset_tensors()
    loop = venv.closed_loop(RandomPartner(SC, seed=9), graph=False, steps=1)
    learner = PPOLearner(seat, lr=1e-3, ent_coef=0.01)
    with pytest.raises(ValueError):                  # nothing recorded, no advantages
        learner.train(sink, n_epochs=1, batch_size=128)
    for _ in range(ST - 1):
        loop.step()
    seat.finish_rollout()
    with pytest.raises(ValueError, match="full"):    # advantages, but one step short
        learner.train(sink, n_epochs=1, batch_size=128)
    loop.step()
    with pytest.raises(ValueError):                  # a plain sink has no advantages
        learner.train(RolloutSink(ST, SN, F, obs_dtype=torch.float32), n_epochs=1)
    seat.finish_rollout()
    # both granules: a permutation of the samples either way; granule 32 keeps tiles of 32 envs together
    for g in (32, 1):
        gen = torch.Generator(device="cuda").manual_seed(3)
        batches = learner.minibatches(sink, 128, granule=g, generator=gen)
        allidx = torch.cat(batches)
        assert [b.numel() for b in batches] == [128] * 4 and allidx.dtype == torch.int32
        assert torch.equal(allidx.sort().values.cpu(), torch.arange(ST * SN, dtype=torch.int32))
        if g == 32:
            tiles = allidx.reshape(-1, 32)
            assert (tiles[:, 0] % 32 == 0).all() and (tiles == tiles[:, :1] + torch.arange(32, device="cuda")).all()
    before = [t.detach().clone() for t in pol.parameters()]
    learner.train(sink, n_epochs=2, batch_size=128, generator=torch.Generator(device="cuda").manual_seed(1))
    learner.train(sink, n_epochs=1, batch_size=100, granule=1)
    stats = learner.stats()
    print("train():", stats)
    assert int(learner.step.item()) == 2 * 4 + 6 and stats["bad"] == 0.0
    assert all(torch.isfinite(t).all() for t in pol.parameters()) and all(np.isfinite(v) for v in stats.values())
    assert all(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
    sink.reset()
    with pytest.raises(ValueError):
        learner.train(sink, n_epochs=1)
