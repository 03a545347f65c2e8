"""-m gpu: the recurrent learner's train sequence (include/oc_policy.h, last section: oc_policy_recurrent_train_step;
``RecurrentPPOLearner.train(shuffle="device")``, ``train_graph``, ``train_stats``) on case c of
tests/recurrent_ppo_ref.py (T = 7, n = 100, F 62, C 16, starts at t = 0, 3, 6: three tiles and a short last cut
of 4 envs): bit parity with the existing update, value clipping against the float64 reference, the KL stop, the
accumulated statistics, a halted step that leaves no trace, and a rollout the closed loop collected.  Every
figure is printed before it is asserted."""
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
import test_recurrent_ppo_gpu as up  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 11
PER = 32                                 # envs per minibatch: 100 envs are cut 32, 32, 32, 4
_bits = up._bits
_shared = {}


def _c():
    """Case c, built once and never changed."""
    if "c" not in _shared:
        _shared["c"] = dict(rp.gpu_cases())["c"]
    return _shared["c"]


def _env(max_groups=0):
    return up._setup(_c(), max_groups=max_groups)


def _state(e):
    ln = e.learner
    return [t.detach().clone() for t in list(ln._params) + [ln.m, ln.v, ln.step, ln.grad_flat, ln.stats_t]
            + list(e.seat._w) + [ln._bwd]]


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _twin_epochs(e, epochs, per, granule, seed, first_epoch=0):
    """The EXISTING update() over the numpy-restated envs; returns each minibatch's stats()."""
    out = []
    for ep in range(first_epoch, first_epoch + epochs):
        envs = rt.epoch_envs(seed, ep, e.n, granule)
        for o, E in rt.env_cuts(e.n, e.T, per):
            e.learner.update(e.sink, torch.from_numpy(envs[o:o + E].copy()).cuda())
            out.append(e.learner.stats())
    return out


# ---- parity with the existing update -------------------------------------------------------------------------------
@pytest.mark.parametrize("granule", [1, 25])
def test_device_train_and_its_graph_are_the_existing_update_bit_for_bit(granule):
    from gym_comm_amd import _lib
    a, twin, g = _env(), _env(), _env()
    assert [E for _, E in rt.env_cuts(a.n, a.T, PER)] == [32, 32, 32, 4]
    a.learner.train(a.sink, n_epochs=2, envs_per_batch=PER, granule=granule, shuffle="device", seed=SEED)
    _twin_epochs(twin, 2, PER, granule, SEED)
    graph = g.learner.train_graph(g.sink, 2, envs_per_batch=PER, granule=granule, seed=SEED)
    assert int(g.learner.step.item()) == 0                  # the warm-up was undone, the capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    first = a.learner._idx.clone()
    assert int(a.learner.step.item()) == 8
    assert _same(_state(a), _state(twin)), "train(shuffle='device') against update() over the restated envs"
    assert _same(_state(a), _state(g)), "one replay against the eager sequence"
    assert torch.equal(a.learner._idx, g.learner._idx)
    assert np.array_equal(first.cpu().numpy(), rt.epoch_envs(SEED, 1, a.n, granule))
    # a second train: the epoch counter went on
    a.learner.train(a.sink, n_epochs=2, envs_per_batch=PER, granule=granule, shuffle="device", seed=SEED)
    graph.replay()
    _twin_epochs(twin, 2, PER, granule, SEED, first_epoch=2)
    torch.cuda.synchronize()
    assert int(a.learner.step.item()) == 16
    assert _same(_state(a), _state(g)) and _same(_state(a), _state(twin))
    assert not torch.equal(a.learner._idx, first) and torch.equal(a.learner._idx, g.learner._idx)
    for e in (a, g):
        words = e.learner.ctl.cpu().tolist()
        assert words[_lib.PPO_CTL["epoch"]] == 4 and words[_lib.PPO_CTL["error"]] == 0
        st = e.learner.train_stats()
        assert st["updates"] == 8 and st["epochs"] == 2 and not st["stopped"]


def test_the_train_variant_of_the_long_case_is_the_existing_update_bit_for_bit():
    """Case d of tests/recurrent_ppo_ref.py (T = 52, E = 129, int8 rows, F + 2 = 32) once through
    oc_policy_recurrent_train_step -- the TRAIN = true instantiations, a unit of their own -- with value clipping
    off and the default plan (256 workgroups, 2 rounds, the second with 4 live items), against update() on a twin."""
    from gym_comm_amd import _lib
    d = up._case("d")[0]
    a, twin = up._setup(d), up._setup(d)
    assert a.learner.plan(a.E, a.T)[:3] == (5, 256, 2) and a.sink.obs.dtype == torch.int8
    ln = a.learner
    assert float(ln.hyper_ext[0].item()) == 0.0               # clip_range_vf off
    before = _state(a)
    _lib.call(ln._L, "oc_policy_recurrent_train_step", ln._dev, ctypes.byref(ln._cfg(a.sink, a.E)),
              ctypes.byref(ln._train_state(a.sink)), a.envs.data_ptr(), a.E)
    twin.learner.update(twin.sink, twin.envs)
    torch.cuda.synchronize()
    names = ["param %d" % i for i in range(len(ln._params))] + ["m", "v", "step", "grad_flat", "stats"] \
        + ["image %d" % i for i in range(len(a.seat._w))] + ["bwd"]
    got, want = _state(a), _state(twin)
    assert len(names) == len(got) == len(want)
    for nm, x, y in zip(names, got, want):
        assert torch.equal(_bits(x), _bits(y)), nm
    assert int(ln.step.item()) == 1 and not _same(got, before)
    assert torch.isfinite(ln.stats_t).all() and ln.stats()["bad"] == 0.0 and ln.grad_flat.abs().max() > 0
    assert ln.ctl.cpu().tolist()[_lib.PPO_CTL["updates"]] == 1


# ---- value clipping --------------------------------------------------------------------------------------------------
def _vclip():
    """The value-clipping tests' inputs and reference, built once: every env of case c in one minibatch, in the
    order of the device permutation of (SEED, epoch 0)."""
    if "v" not in _shared:
        base = _c()
        envs = rt.epoch_envs(SEED, 0, base["n"], 1)
        case = dict(base, envs=envs)
        old_v = rt.recorded_values(base)
        hp = rp.test_hp()
        _shared["v"] = dict(case=case, envs=envs, old_v=old_v, hp=hp,
                            ref=rt.clipped_loss_and_grad(case, old_v, rt.C_VF, hp),
                            plain=rp.loss_and_grad(case, hp), cond=rt.gate_conditions(case, old_v, rt.C_VF))
    return _shared["v"]


def _venv(max_groups):
    v = _vclip()
    e = up._setup(v["case"], max_groups=max_groups)
    e.sink.values.copy_(torch.from_numpy(v["old_v"]))
    return e


@pytest.mark.parametrize("max_groups", [0, 1])
def test_value_clipping_against_the_reference_and_switched_by_a_device_write(max_groups):
    v = _vclip()
    c = rt.C_VF
    ref, rstats, info = v["ref"]
    print("clip_range_vf %.3f: open gates %.3f, min | |v - old_v| - c | %.4f" % ((c,) + v["cond"]))
    assert 0.3 <= v["cond"][0] <= 0.7 and v["cond"][1] > 0.05
    e = _venv(max_groups)
    ln = e.learner
    ln.set_clip_range_vf(c)
    graph = ln.train_graph(e.sink, 1, envs_per_batch=None, granule=1, seed=SEED)
    start = [t.clone() for t in ln._train_tensors()]
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ln._idx.cpu().numpy(), v["envs"])
    assert ln.plan(e.n, e.T)[1] == (1 if max_groups else 28)
    got = {k: g.detach().cpu().numpy().astype(np.float64) for k, g in ln.grads.items()}
    stats = ln.stats()
    clipped_bits = _bits(ln.grad_flat).clone()
    d, sd = rp.rel_diff(got, ref), rp.stats_diff(stats, rstats)
    print("max_groups", max_groups, "grad", {k: "%.3g" % x for k, x in d.items()}, "largest %.3g" % max(d.values()))
    print("max_groups", max_groups, "stats", {k: "%.3g" % x for k, x in sd.items()}, "largest %.3g" % max(sd.values()))
    plain_vl = rp.stats_diff(stats, v["plain"][1], ("value_loss",))["value_loss"]
    plain_g = max(rp.rel_diff(got, v["plain"][0]).values())
    print("against the UNCLIPPED reference: value_loss %.3g, gradient %.3g" % (plain_vl, plain_g))
    assert max(d.values()) <= rp.TOL_G, d
    assert max(sd.values()) <= rp.TOL_S, sd
    assert plain_vl > rp.TOL_S and plain_g > rp.TOL_G      # the unclipped loss lies outside the tolerance here
    for m in rt.VCLIP_MUTANTS:
        mref = rt.clipped_loss_and_grad(v["case"], v["old_v"], c, v["hp"], mutate=m)[0]
        assert max(rp.rel_diff(got, mref).values()) > rp.TOL_G, m
    # eager gives the captured sequence's bits
    twin = _venv(max_groups)
    twin.learner.set_clip_range_vf(c)
    twin.learner.train(twin.sink, n_epochs=1, granule=1, shuffle="device", seed=SEED)
    torch.cuda.synchronize()
    assert _same(_state(e), _state(twin))
    # clipping switched off by a device write, the SAME graph: the existing update's bits
    with torch.no_grad():
        for t, s in zip(ln._train_tensors(), start):
            t.copy_(s)
    ln.set_clip_range_vf(None)
    graph.replay()
    off = _venv(max_groups)
    off.learner.update(off.sink, torch.from_numpy(v["envs"].copy()).cuda())
    torch.cuda.synchronize()
    assert _same(_state(e), _state(off))
    assert not torch.equal(_bits(ln.grad_flat), clipped_bits)


# ---- the KL stop and the accumulated statistics ----------------------------------------------------------------------
def _one_epoch():
    """One epoch of 32, 32, 32, 4 envs by the existing update(): its state, and each minibatch's stats()."""
    if "kl" not in _shared:
        twin = _env()
        per = _twin_epochs(twin, 1, PER, 1, SEED)
        kl = [np.float64(np.float32(s["approx_kl"])) for s in per]
        m = np.float64(0.0)
        for x in kl:
            m += x
        torch.cuda.synchronize()
        _shared["kl"] = dict(state=_state(twin), per=per, mean=float(m / np.float64(len(kl))))
        print("approx_kl per minibatch", kl, "mean", _shared["kl"]["mean"])
    return _shared["kl"]


@pytest.mark.parametrize("captured", [False, True])
def test_kl_rule_stops_after_the_epoch_whose_mean_exceeds_the_target(captured):
    ref = _one_epoch()
    m = ref["mean"]
    assert len(ref["per"]) == 4 and m > 0

    def run(target):
        e = _env()
        e.learner.set_target_kl(target)
        if captured:
            e.learner.train_graph(e.sink, 3, envs_per_batch=PER, granule=1, seed=SEED).replay()
        else:
            e.learner.train(e.sink, n_epochs=3, envs_per_batch=PER, granule=1, shuffle="device", seed=SEED)
        torch.cuda.synchronize()
        return e, e.learner.train_stats()

    e, st = run(m / 1.5 * (1 - 1e-3))                       # 1.5 target just below the mean: stop
    print("just below:", st)
    assert st["stopped"] and st["epochs"] == 1 and st["updates"] == 4 and int(e.learner.step.item()) == 4
    assert _same(_state(e), ref["state"])                   # bit for bit a one-epoch train
    e, st = run(m / 1.5 * (1 + 1e-3))                       # just above: the second epoch runs
    print("just above:", st)
    assert st["epochs"] >= 2 and st["updates"] >= 8 and int(e.learner.step.item()) == st["updates"]
    assert not _same(_state(e), ref["state"])


def test_train_stats_are_the_means_of_the_minibatches_statistics():
    twin, e = _env(), _env()
    per = _twin_epochs(twin, 2, PER, 1, SEED)
    e.learner.train(e.sink, n_epochs=2, envs_per_batch=PER, granule=1, shuffle="device", seed=SEED)
    st = e.learner.train_stats()
    print(st)
    assert st["updates"] == len(per) == 8 and st["epochs"] == 2 and not st["stopped"]
    for k in tr.TRAIN_STATS:
        terms = np.array([np.float64(np.float32(s[k])) for s in per])
        want = terms.mean()
        print(k, "train_stats %.12g mean of stats() %.12g" % (st[k], want))
        assert abs(st[k] - want) <= 2 * pp.U * np.abs(terms).mean(), k


# ---- a halted sequence leaves no trace -------------------------------------------------------------------------------
@pytest.mark.parametrize("word", ["stop", "error"])
def test_a_halted_train_step_writes_nothing(word):
    from gym_comm_amd import _lib
    e = _env()
    ln, E = e.learner, e.E
    ln.lp_out = torch.full((e.T * E,), 7.0, device="cuda")
    ln.v_out = torch.full((e.T * E,), 7.0, device="cuda")
    ln.update(e.sink, e.envs)                               # real numbers everywhere, the scratch allocated
    ln.ctl[_lib.PPO_CTL[word]] = 1
    ln.acc.fill_(3.0)
    ln.stats_t.fill_(5.0)
    ln.lp_out.fill_(7.0)
    ln.v_out.fill_(9.0)
    watched = lambda: _state(e) + [ln._scratch.clone(), ln._train_words.clone(), ln.lp_out.clone(), ln.v_out.clone()]  # noqa: E731
    before = watched()
    step = lambda: _lib.call(ln._L, "oc_policy_recurrent_train_step", ln._dev, ctypes.byref(ln._cfg(e.sink, E)),  # noqa: E731
                             ctypes.byref(ln._train_state(e.sink)), e.envs.data_ptr(), E)
    step()
    torch.cuda.synchronize()
    assert int(ln.step.item()) == 1 and _same(before, watched())
    ln.ctl[_lib.PPO_CTL[word]] = 0                          # and it was the word that held it back
    step()
    torch.cuda.synchronize()
    assert int(ln.step.item()) == 2 and not _same(before, watched())
    assert ln.ctl.cpu().tolist()[_lib.PPO_CTL["updates"]] == 1


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_a_captured_train_replays_on_rollouts_collected_by_the_closed_loop():
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
    learner = RecurrentPPOLearner(seat, lr=1e-3, ent_coef=0.0, vf_coef=1e-3, clip_range_vf=0.2, target_kl=None)
    graph = None
    for rollout in (1, 2):
        seat.begin_rollout()
        for _ in range(ST):
            loop.step()
        seat.finish_rollout()
        if graph is None:
            with pytest.raises(ValueError, match="shuffle"):
                learner.train(sink, n_epochs=1, shuffle="nonsense")
            graph = learner.train_graph(sink, 2, envs_per_batch=32)
            assert int(learner.step.item()) == 0
        before = [t.detach().clone() for t in pol.parameters()]
        graph.replay()
        torch.cuda.synchronize()
        st, last = learner.train_stats(), learner.stats()
        print("rollout", rollout, st)
        assert st["updates"] == 4 and st["epochs"] == 2 and not st["stopped"] and last["bad"] == 0.0
        assert all(np.isfinite(x) for x in st.values()) and all(np.isfinite(x) for x in last.values())
        assert all(torch.isfinite(t).all() for t in pol.parameters())
        assert all(not torch.equal(a, b) for a, b in zip(before, pol.parameters()))
        assert int(learner.step.item()) == 4 * rollout
    assert int(learner.step.item()) == 8
    loop.step()                                              # the seat acts afterwards, on the new images
    assert torch.isfinite(seat.log_prob).all() and torch.isfinite(seat.value).all()
