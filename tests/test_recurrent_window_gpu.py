"""-m gpu: windows of a rollout (include/oc_policy.h, "windows of a rollout"; ``RolloutSink(state_window=W)``,
``FusedRecurrentPartner``'s snapshot, ``RecurrentPPOLearner.update_windows`` / ``train_windows`` /
``train_graph_windows``).  Both kernels are copies and the update behind them is the unchanged one, so every check
here is bit for bit: the snapshot and the gather against torch indexing, the windowed update against the existing
update on a plain sink of W slots and E envs built by torch indexing, the recorded states against the seat's own,
and the windowed train sequence against hand-driven ``update_windows`` calls over the restated permutation."""
import copy
import ctypes
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
import ppo_train_ref as tr  # noqa: E402
import recurrent_ppo_ref as rp  # noqa: E402
import recurrent_train_ref as rt  # noqa: E402

pytestmark = pytest.mark.gpu
DT = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}
SENTINEL = -7.0
_CASES = {}


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _eq(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _case(name):
    """The synthetic sinks, built once and never changed: ``f`` float32 rows, T = 6, n = 80, F = 29, C = 5, starts at
    t = 0, 1, 3; ``i`` int8 rows, T = 4, n = 40, F = 14, C = 1; ``q`` T = 6, n = 40, starts at t = 0 only (windows 1
    and 2 of three hold none); ``t`` T = 4, n = 64, starts at t = 0, 1, 3, for the train sequence."""
    if not _CASES:
        _CASES["f"] = rp.make_case(6, 80, np.arange(80), 29, 5, "float32", 21, starts=(0, 1, 3))
        _CASES["i"] = rp.make_case(4, 40, np.arange(40), 14, 1, "int8", 22, starts=(0, 3))
        _CASES["q"] = rp.make_case(6, 40, np.arange(40), 14, 1, "int32", 23, starts=(0,))
        _CASES["t"] = rp.make_case(4, 64, np.arange(64), 14, 1, "int8", 24, starts=(0, 1, 3))
    return _CASES[name]


def _put(t, a):
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def _setup(case, W, hp=None, **kw):
    """``tests/test_recurrent_ppo_gpu._setup`` with a sink that has windows: the case's tensors in a full,
    chronological ``RolloutSink(state_window=W)``, ``lstm_states`` random (states[0] the case's h0 / c0), recorded
    values away from the current ones (``recurrent_train_ref.recorded_values``)."""
    from gym_comm_amd.vec_env import FusedRecurrentPartner, RecurrentPPOLearner, RolloutSink
    hp = hp or rp.test_hp()
    T, F, n = case["obs"].shape
    pol = copy.deepcopy(case["pol"]).float().cuda()
    seat = FusedRecurrentPartner(pol, sample=True, seed=5)
    sink = RolloutSink(T, n, F, obs_dtype=DT[case["odt"]], fused=True, state_window=W)
    _put(sink.obs, case["obs"]), _put(sink.timestep, case["ts"]), _put(sink.actions, case["actions"])
    _put(sink.log_probs, case["old_lp"]), _put(sink.advantages, case["adv"]), _put(sink.returns, case["ret"])
    _put(sink.episode_starts, case["es"])
    if "old_v" not in case:
        case["old_v"] = rt.recorded_values(case)
    _put(sink.values, case["old_v"])
    if W is not None:
        states = np.random.default_rng(500 + T).uniform(-1, 1, (T // W, 2, 64, n)).astype(np.float32)
        states[0, 0], states[0, 1] = case["h0"], case["c0"]
        _put(sink.lstm_states, states)
    sink.count.fill_(T)
    sink.returns_ready = True
    seat.begin_rollout(n)
    _put(seat.h0, case["h0"]), _put(seat.c0, case["c0"])
    learner = RecurrentPPOLearner(seat, lr=hp.lr, clip_range=hp.clip, ent_coef=hp.ent, vf_coef=hp.vf,
                                  max_grad_norm=hp.max_norm, betas=(hp.b1, hp.b2), eps=hp.eps, **kw)
    return SimpleNamespace(case=case, hp=hp, pol=pol, seat=seat, sink=sink, learner=learner, T=T, n=n, F=F, W=W)


def _plain(e, seqs, **kw):
    """A second, plain sink of W slots and E envs built by torch indexing from ``e.sink`` for the sequence ids
    ``seqs``, its seat's h0 / c0 the recorded states, and a learner of its own on a copy of the same module."""
    from gym_comm_amd.vec_env import FusedRecurrentPartner, RecurrentPPOLearner, RolloutSink
    W, n, hp = e.W, e.n, e.hp
    s = seqs.long()
    k, env = s // n, s % n
    E = s.numel()
    slots = k.unsqueeze(0) * W + torch.arange(W, device="cuda").unsqueeze(1)          # [W][E]
    sink2 = RolloutSink(W, E, e.F, obs_dtype=e.sink.obs.dtype, fused=True)
    for name in ("timestep", "log_probs", "advantages", "returns", "episode_starts", "values"):
        getattr(sink2, name).copy_(getattr(e.sink, name)[slots, env.unsqueeze(0)])
    for t in range(W):
        sink2.obs[t].copy_(e.sink.obs[k * W + t, :, env].T)
        sink2.actions[t].copy_(e.sink.actions[k * W + t, :, env].T)
    sink2.count.fill_(W)
    sink2.returns_ready = True
    pol = copy.deepcopy(e.case["pol"]).float().cuda()
    seat = FusedRecurrentPartner(pol, sample=True, seed=5)
    seat.begin_rollout(E)
    seat.h0.copy_(e.sink.lstm_states[k, 0, :, env].T)
    seat.c0.copy_(e.sink.lstm_states[k, 1, :, env].T)
    learner = RecurrentPPOLearner(seat, lr=hp.lr, clip_range=hp.clip, ent_coef=hp.ent, vf_coef=hp.vf,
                                  max_grad_norm=hp.max_norm, betas=(hp.b1, hp.b2), eps=hp.eps, **kw)
    return SimpleNamespace(pol=pol, seat=seat, sink=sink2, learner=learner, E=E,
                           envs=torch.arange(E, dtype=torch.int32, device="cuda"))


def _state(ln, seat):
    return [t.detach().clone() for t in list(ln._params) + [ln.m, ln.v, ln.step, ln.grad_flat, ln.stats_t]
            + list(seat._w) + [ln._bwd]]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _subset(count, size, seed):
    """``size`` shuffled sequence ids out of ``count``, the last one a repeat of the first."""
    ids = np.random.default_rng(seed).permutation(count)[:size - 1]
    return torch.from_numpy(np.concatenate([ids, ids[:1]]).astype(np.int32)).cuda()


# ---- 1. the snapshot ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [80, 1, 4099, 12289])
def test_the_snapshot_copies_exactly_where_a_window_begins(n, aligned):
    """T = 6, W = 3: pos 0 and 6 (wraps) write states[0], pos 3 writes states[1], pos 1 and 5 write nothing.  n = 1 and
    4 099 are single and odd row lengths; ``aligned=False`` hands h over 4 bytes past a 16-byte boundary, which takes
    the scalar path for everything.  n = 12 289 is beyond the cap of 1 024 workgroups: the 64 n / 2 float4 pairs ask
    for 1 537, so the strided loop's second pass is partly full (the scalar path asks for 3 073: three full passes and
    64 elements of a fourth)."""
    from gym_comm_amd import _lib
    L = _lib.load(lib="policy")
    T, W = 6, 3
    g = torch.Generator(device="cuda").manual_seed(n)
    store = torch.rand(64 * n + 1, device="cuda", generator=g)
    h = (store[:-1] if aligned else store[1:]).view(64, n)
    c = torch.rand((64, n), device="cuda", generator=g) + 2.0
    assert (h.data_ptr() % 16 == 0) == aligned
    states = torch.full((T // W + 1, 2, 64, n), SENTINEL, device="cuda")                  # the last block: a guard band
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    for p, k in ((0, 0), (1, None), (3, 1), (5, None), (6, 0)):
        states.fill_(SENTINEL)
        pos.fill_(p)
        _lib.call(L, "oc_policy_window_snapshot", 0, pos.data_ptr(), T, W, h.data_ptr(), c.data_ptr(), states.data_ptr(), n)
        torch.cuda.synchronize()
        for j in range(T // W + 1):
            if j == k:
                assert _eq(states[j, 0], h) and _eq(states[j, 1], c), (p, j)
            else:
                assert (states[j] == SENTINEL).all(), (p, j)
        assert int(pos.item()) == p


# ---- 2. the gather -------------------------------------------------------------------------------------------------
def _gather_raw(e, seqs, extra=3):
    """The gather into a window batch with room for ``extra`` sequences more than E: what lies behind the first E
    sequences' worth of every tensor is a guard band."""
    from gym_comm_amd import _lib, learner
    ln = e.learner
    E = seqs.numel()
    b = learner._WindowBatch(e.W, e.F, E + extra, e.sink.obs.dtype, "cuda")
    for t in b.tensors():
        t.fill_(SENTINEL)
    _lib.call(ln._L, "oc_policy_window_gather", 0, ctypes.byref(ln._window_src(e.sink)), ctypes.byref(b.c_struct),
              seqs.data_ptr(), E)
    torch.cuda.synchronize()
    return b


@pytest.mark.parametrize("name,W,E", [("f", 3, 67), ("i", 2, 67), ("f", 3, 1), ("i", 2, 1)])
def test_the_gather_is_torch_indexing_bit_for_bit(name, W, E):
    e = _setup(_case(name), W)
    count = e.learner.sequences(e.sink)
    assert count == e.n * e.T // W
    seqs = _subset(count, E, 7) if E > 1 else torch.tensor([count - 1], dtype=torch.int32, device="cuda")
    b = _gather_raw(e, seqs)
    k, env = seqs.long() // e.n, seqs.long() % e.n
    if E > 1:
        assert E % 32 and seqs[-1] == seqs[0] and len(set(k.tolist())) == e.T // W
    sink = e.sink
    for t in range(W):
        slot = k * W + t
        assert _eq(b.view("obs", E)[t], sink.obs[slot, :, env].T), t
        assert _eq(b.view("actions", E)[t], sink.actions[slot, :, env].T), t
        for nm in ("timestep", "log_probs", "advantages", "returns", "episode_starts", "values"):
            assert _eq(b.view(nm, E)[t], getattr(sink, nm)[slot, env]), (nm, t)
    assert _eq(b.view("h0", E), sink.lstm_states[k, 0, :, env].T) and _eq(b.view("c0", E), sink.lstm_states[k, 1, :, env].T)
    for nm in ("obs", "timestep", "actions", "log_probs", "advantages", "returns", "episode_starts", "values", "h0", "c0"):
        used = b.view(nm, E).numel()
        band = getattr(b, nm)[used:]
        assert band.numel() > 0 and (band == SENTINEL).all(), nm                      # untouched behind the E sequences
    assert torch.isfinite(b.view("log_probs", E)).all() and (E == 1 or (b.view("episode_starts", E) > 0).any())


# ---- 3. the windowed update is the unchanged update on the gathered data ----------------------------------------------
@pytest.mark.parametrize("name,W", [("f", 3), ("i", 2)])
def test_the_windowed_update_is_the_existing_update_on_a_plain_sink_of_the_gathered_data(name, W):
    e = _setup(_case(name), W)
    seqs = _subset(e.learner.sequences(e.sink), 67, 7)
    p = _plain(e, seqs)
    E = p.E
    for side, ln in ((e, e.learner), (p, p.learner)):
        ln.lp_out, ln.v_out = torch.full((W, E), 7.0, device="cuda"), torch.full((W, E), 7.0, device="cuda")
    e.learner.grad_windows(e.sink, seqs)
    p.learner.grad(p.sink, p.envs)
    torch.cuda.synchronize()
    assert _eq(e.learner.grad_flat, p.learner.grad_flat) and _eq(e.learner.stats_t, p.learner.stats_t)
    assert _eq(e.learner.lp_out, p.learner.lp_out) and _eq(e.learner.v_out, p.learner.v_out)
    assert torch.isfinite(e.learner.lp_out).all() and e.learner.grad_flat.abs().max() > 0
    assert e.learner.plan(E, W)[6] == 6                                                # six launches behind the gather
    for i in range(3):
        e.learner.update_windows(e.sink, seqs)
        p.learner.update(p.sink, p.envs)
        torch.cuda.synchronize()
        assert _same(_state(e.learner, e.seat), _state(p.learner, p.seat)), i
    assert int(e.learner.step.item()) == 3


# ---- 4. the recorded states are the right ones, end to end ------------------------------------------------------------
def _rollout(captured, warmup):
    from gym_comm_amd.vec_env import (FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RandomPartner,
                                      RolloutSink)
    SC, ST, SN, W = 2, 8, 64, 4
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=5, ego_config={},
                          partner_config={}, num_communication=SC, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, SN, seed=5, obs_dtype=torch.float32)
    F = 22 + venv._b.S + 2 * SC
    pol = LSTMActorCritic(venv._b.S, SC, seed=31).cuda()
    sink = RolloutSink(ST, SN, F, obs_dtype=torch.float32, fused=True, state_window=W)
    venv.partner = seat = FusedRecurrentPartner(pol, sample=True, seed=12, sink=sink)
    venv.reset_tensors()
    loop = venv.closed_loop(RandomPartner(SC, seed=9), graph=captured, steps=W if captured else 1)
    for _ in range(warmup):
        loop.enqueue()
    seat.begin_rollout()
    sink.lstm_states.fill_(SENTINEL)
    clones = []
    if captured:
        for _ in range(ST // W):
            loop.step()
    else:
        for t in range(ST):
            if t % W == 0:
                clones.append((seat.h.clone(), seat.c.clone()))
            loop.step()
    seat.finish_rollout()
    torch.cuda.synchronize()
    return SimpleNamespace(venv=venv, seat=seat, sink=sink, pol=pol, clones=clones, W=W, T=ST, n=SN, loop=loop)


@pytest.mark.parametrize("warmup", [3, 1])
def test_the_seat_records_the_state_before_every_windows_first_step(warmup):
    """64 envs whose episodes last 5 steps, 8 recorded steps in windows of 4.  After 3 warm-up steps the episodes start
    in slots 2 and 7 -- inside both windows; after 1 warm-up step in slot 4 -- where window 1 begins."""
    from gym_comm_amd.vec_env import RecurrentPPOLearner
    a = _rollout(False, warmup)
    es = a.sink.episode_starts
    slots = [t for t in range(a.T) if bool((es[t] > 0).any())]
    print("warm-up", warmup, "episode starts in slots", slots)
    if warmup == 3:
        assert any(t % a.W for t in slots) and bool((es[2] > 0).all()) and bool((es[7] > 0).all())
    else:
        assert slots == [4] and bool((es[4] > 0).all())
    assert int(a.sink.pos.item()) == 0 and a.sink.steps() == a.T
    for k, (h, c) in enumerate(a.clones):
        assert _eq(a.sink.lstm_states[k, 0], h) and _eq(a.sink.lstm_states[k, 1], c), k
    assert _eq(a.sink.lstm_states[0, 0], a.seat.h0) and _eq(a.sink.lstm_states[0, 1], a.seat.c0)
    assert a.sink.lstm_states[1].abs().max() > 0 and not (a.sink.lstm_states == SENTINEL).any()
    # the captured closed loop picks the snapshot up: the same bits
    g = _rollout(True, warmup)
    assert g.loop.graph is not None
    for nm in ("lstm_states", "obs", "actions", "log_probs", "values", "episode_starts", "advantages", "returns"):
        assert _eq(getattr(a.sink, nm), getattr(g.sink, nm)), nm
    assert _eq(a.seat.h, g.seat.h) and _eq(a.seat.c, g.seat.c) and _eq(a.seat.h0, g.seat.h0)
    # with unchanged weights the windows' forward is the whole sequences' forward, row for row
    ln = RecurrentPPOLearner(a.seat)
    full_lp, full_v = torch.full((a.T, a.n), 7.0, device="cuda"), torch.full((a.T, a.n), 7.0, device="cuda")
    ln.lp_out, ln.v_out = full_lp, full_v
    ln.grad(a.sink, torch.arange(a.n, dtype=torch.int32, device="cuda"))
    count = ln.sequences(a.sink)
    assert count == 128
    win_lp, win_v = torch.full((a.W, count), 9.0, device="cuda"), torch.full((a.W, count), 9.0, device="cuda")
    ln.lp_out, ln.v_out = win_lp, win_v
    ln.grad_windows(a.sink, torch.arange(count, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    K = a.T // a.W
    assert _eq(win_lp.view(a.W, K, a.n).permute(1, 0, 2).reshape(a.T, a.n), full_lp)
    assert _eq(win_v.view(a.W, K, a.n).permute(1, 0, 2).reshape(a.T, a.n), full_v)
    assert torch.isfinite(full_lp).all() and ln.stats()["bad"] == 0.0


# ---- 5. truncation -----------------------------------------------------------------------------------------------------
def test_a_windows_start_state_is_its_own_and_nothing_flows_across_its_first_step():
    case = _case("q")
    assert case["es"][0].any() and not case["es"][1:].any()                            # no start in windows 1 and 2
    e = _setup(case, 2)
    n = e.n
    envs = np.random.default_rng(3).permutation(n)[:33]
    window0 = torch.from_numpy(envs.astype(np.int32)).cuda()                           # ids of window 0: k n + env, k = 0
    mixed = torch.from_numpy(np.concatenate([envs[:20], n + envs[:13]]).astype(np.int32)).cuda()   # ... and of window 1

    def grads(seqs):
        e.learner.grad_windows(e.sink, seqs)
        torch.cuda.synchronize()
        return e.learner.grad_flat.clone(), e.learner.stats_t.clone()
    g0, s0 = grads(window0)
    g1, s1 = grads(mixed)
    e.sink.lstm_states[1][:, :, torch.from_numpy(envs).cuda()] += 0.25                # the minibatches' envs, window 1
    h0, t0 = grads(window0)
    h1, t1 = grads(mixed)
    assert _eq(g0, h0) and _eq(s0, t0)              # window 0 ends where window 1's state was recorded: not a bit moves
    assert not _eq(g1, h1) and (g1 - h1).abs().max() > 1e-6 * g1.abs().max()
    # ... and window 1's samples see window 0's steps only through that state: window 0's data does not reach them
    only1 = torch.from_numpy((n + envs).astype(np.int32)).cuda()
    g2, _ = grads(only1)
    e.sink.obs[0:2] = 0
    e.sink.episode_starts[0:2] = 1.0
    h2, _ = grads(only1)
    assert _eq(g2, h2)


# ---- 6. the train sequence ---------------------------------------------------------------------------------------------
SEED, PER, GRANULE = 11, 48, 32


def _tenv(**kw):
    return _setup(_case("t"), 2, **kw)


def _hand_epochs(e, epochs, first_epoch=0):
    """``update_windows`` over the numpy-restated permutation of the sequence ids; each minibatch's stats()."""
    from gym_comm_amd import learner
    count = e.learner.sequences(e.sink)
    out = []
    for ep in range(first_epoch, first_epoch + epochs):
        seqs = rt.epoch_envs(SEED, ep, count, GRANULE)
        for o, E in learner.sequence_cuts(count, e.W, PER):
            e.learner.update_windows(e.sink, torch.from_numpy(seqs[o:o + E].copy()).cuda())
            out.append(e.learner.stats())
    return out


def test_device_train_over_windows_and_its_graph_are_update_windows_bit_for_bit():
    from gym_comm_amd import _lib, learner
    a, twin, g = _tenv(), _tenv(), _tenv()
    count = a.learner.sequences(a.sink)
    assert count == 128 and [E for _, E in learner.sequence_cuts(count, 2, PER)] == [48, 48, 32]
    a.learner.train_windows(a.sink, n_epochs=2, sequences_per_batch=PER, granule=GRANULE, shuffle="device", seed=SEED)
    per = _hand_epochs(twin, 2)
    graph = g.learner.train_graph_windows(g.sink, 2, sequences_per_batch=PER, granule=GRANULE, seed=SEED)
    assert int(g.learner.step.item()) == 0                  # the warm-up was undone, the capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    first = a.learner._idx.clone()
    assert int(a.learner.step.item()) == 6
    assert _same(_state(a.learner, a.seat), _state(twin.learner, twin.seat)), "train_windows against update_windows"
    assert _same(_state(a.learner, a.seat), _state(g.learner, g.seat)), "one replay against the eager sequence"
    assert np.array_equal(first.cpu().numpy(), rt.epoch_envs(SEED, 1, count, GRANULE))
    tiles = first.view(-1, GRANULE).long()
    assert (tiles[:, -1] - tiles[:, 0] == GRANULE - 1).all() and (tiles[:, 0] // a.n == tiles[:, -1] // a.n).all()
    st = a.learner.train_stats()
    print(st)
    assert st["updates"] == len(per) == 6 and st["epochs"] == 2 and not st["stopped"]
    for k in tr.TRAIN_STATS:                                 # the train variant's sums against the per-update stats()
        terms = np.array([np.float64(np.float32(s[k])) for s in per])
        print(k, "train_stats %.12g mean of stats() %.12g" % (st[k], terms.mean()))
        assert abs(st[k] - terms.mean()) <= 2 * pp.U * np.abs(terms).mean(), k
    # a second train, a second replay: the epoch counter went on
    a.learner.train_windows(a.sink, n_epochs=2, sequences_per_batch=PER, granule=GRANULE, shuffle="device", seed=SEED)
    graph.replay()
    _hand_epochs(twin, 2, first_epoch=2)
    torch.cuda.synchronize()
    assert int(a.learner.step.item()) == 12
    assert _same(_state(a.learner, a.seat), _state(g.learner, g.seat))
    assert _same(_state(a.learner, a.seat), _state(twin.learner, twin.seat))
    assert not torch.equal(a.learner._idx, first) and torch.equal(a.learner._idx, g.learner._idx)
    assert a.learner.ctl.cpu().tolist()[_lib.PPO_CTL["epoch"]] == 4
    # the torch shuffle covers every sequence once per epoch
    mb = a.learner.minibatches_windows(a.sink, PER, GRANULE, torch.Generator(device="cuda").manual_seed(1))
    assert [b.numel() for b in mb] == [48, 48, 32] and sorted(torch.cat(mb).tolist()) == list(range(count))
    a.learner.train_windows(a.sink, n_epochs=1, sequences_per_batch=PER, granule=GRANULE)
    assert int(a.learner.step.item()) == 15


def test_the_kl_rule_stops_the_windowed_sequence_after_the_first_epoch():
    def env():
        e = _tenv()
        e.sink.log_probs.add_(0.5)                            # approx_kl = mean(old_lp - lp) is positive whatever happens
        return e
    twin = env()
    per = _hand_epochs(twin, 1)
    kl = np.mean([s["approx_kl"] for s in per])
    print("approx_kl per minibatch", [s["approx_kl"] for s in per])
    assert kl > 0.05
    torch.cuda.synchronize()
    for captured in (False, True):
        e = env()
        e.learner.set_target_kl(1e-6)
        if captured:
            e.learner.train_graph_windows(e.sink, 3, sequences_per_batch=PER, granule=GRANULE, seed=SEED).replay()
        else:
            e.learner.train_windows(e.sink, n_epochs=3, sequences_per_batch=PER, granule=GRANULE, shuffle="device", seed=SEED)
        torch.cuda.synchronize()
        st = e.learner.train_stats()
        print("captured", captured, st)
        assert st["stopped"] and st["epochs"] == 1 and st["updates"] == 3 and int(e.learner.step.item()) == 3
        assert _same(_state(e.learner, e.seat), _state(twin.learner, twin.seat))


def test_value_clipping_clips_about_the_gathered_recorded_values():
    from gym_comm_amd import _lib
    c = rt.C_VF

    def run(clip):
        e = _tenv(clip_range_vf=clip)
        e.learner.train_windows(e.sink, n_epochs=1, sequences_per_batch=None, granule=GRANULE, shuffle="device", seed=SEED)
        torch.cuda.synchronize()
        return e
    on, off = run(c), run(None)
    s_on, s_off = on.learner.stats(), off.learner.stats()
    print("value_loss clipped %.9g unclipped %.9g" % (s_on["value_loss"], s_off["value_loss"]))
    assert abs(s_on["value_loss"] - s_off["value_loss"]) > 1e-3 and not _eq(on.learner.grad_flat, off.learner.grad_flat)
    assert torch.equal(on.learner._idx, off.learner._idx)
    # the same minibatch on the plain W x E sink, through the train step by hand
    seqs = on.learner._idx[:128].clone()
    p = _plain(_tenv(), seqs, clip_range_vf=c)
    ln = p.learner
    _lib.call(ln._L, "oc_policy_recurrent_train_step", ln._dev, ctypes.byref(ln._cfg(p.sink, p.E)),
              ctypes.byref(ln._train_state(p.sink)), p.envs.data_ptr(), p.E)
    torch.cuda.synchronize()
    assert _same(_state(on.learner, on.seat), _state(ln, p.seat))
    assert on.learner.train_stats()["value_loss"] == ln.train_stats()["value_loss"]


# ---- 7. nothing new without windows ------------------------------------------------------------------------------------
def test_without_windows_the_seat_and_the_learner_launch_what_they_launched(monkeypatch):
    from gym_comm_amd import _lib
    from gym_comm_amd.vec_env import RolloutSink
    calls = []
    real = _lib.call

    def recording(L, name, *args, **kw):
        calls.append(name)
        return real(L, name, *args, **kw)
    monkeypatch.setattr(_lib, "call", recording)
    case = _case("t")
    rows = torch.from_numpy(case["obs"][0]).cuda()
    obs = SimpleNamespace(rows=rows, timestep=torch.from_numpy(case["ts"][0]).cuda())
    for W, want in ((None, ["oc_policy_lstm_ac", "oc_rollout_add"]),
                    (2, ["oc_policy_window_snapshot", "oc_policy_lstm_ac", "oc_rollout_add"])):
        e = _setup(case, W)
        e.seat.sink = sink = RolloutSink(e.T, e.n, e.F, obs_dtype=torch.int8, fused=True, state_window=W)
        assert (sink.lstm_states is None) == (W is None) and sink.state_window == W and len(sink.get_state()) == (3 if W is None else 4)
        mv, cm = torch.zeros(e.n, dtype=torch.int32, device="cuda"), torch.zeros(e.n, dtype=torch.int32, device="cuda")
        del calls[:]
        e.seat.act_into(obs, mv, cm)
        assert calls == want, calls
    e = _setup(case, None)
    assert e.sink.lstm_states is None
    del calls[:]
    e.learner.train(e.sink, n_epochs=1, envs_per_batch=32, granule=32, shuffle="device", seed=SEED)
    e.learner.train(e.sink, n_epochs=1, envs_per_batch=32, granule=32)
    torch.cuda.synchronize()
    assert not any("window" in c for c in calls) and e.learner._wbatch is None and not e.learner._wsrcs
    assert calls[:4] == ["oc_policy_ppo_train_begin", "oc_policy_ppo_epoch_begin", "oc_policy_recurrent_train_step",
                         "oc_policy_recurrent_train_step"] and calls[4:] == ["oc_policy_rppo_update"] * 2
    with pytest.raises(ValueError, match="state_window"):
        e.learner.train_windows(e.sink, n_epochs=1)
    w = _setup(case, 2)
    del calls[:]
    w.learner.update_windows(w.sink, torch.arange(40, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert calls == ["oc_policy_window_gather", "oc_policy_rppo_update"] and w.learner._wbatch.cap == 40
    first = w.learner._wbatch
    w.learner.update_windows(w.sink, torch.arange(64, dtype=torch.int32, device="cuda"))       # regrows by retiring
    assert w.learner._wbatch is not first and any(r is first for r in w.learner._retired)
    w.learner.update_windows(w.sink, torch.arange(8, dtype=torch.int32, device="cuda"))        # fits: the same batch
    torch.cuda.synchronize()
    assert w.learner._wbatch.cap == 64 and int(w.learner.step.item()) == 3
