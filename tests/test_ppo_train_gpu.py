"""GPU: the train sequence (include/oc_policy.h, the last section; PPOLearner.train(shuffle="device"),
train_graph, train_stats) on ppo_ref.make_buffer's sink of T = 3 slots x n = 70 envs: the shuffle
kernel against the host permutation, bit parity with the existing update, value clipping against the
float64 reference and its derived bounds, the KL stop, the accumulated statistics, and a halted
sequence that leaves no trace.  Every figure is printed before it is asserted."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ppo_ref as pp  # noqa: E402
import ppo_train_ref as tr  # noqa: E402
import test_ppo_update_gpu as up  # noqa: E402

pytestmark = pytest.mark.gpu
TOTAL = pp.T_SLOTS * pp.N_ENVS
F, C, ODT, SCALE, _, _, SEED = tr.VCASE
SHUFFLE_SEED = 11
_bits = up._bits


def _env(max_groups=0):
    """test_ppo_update_gpu's setup with the sink marked full and its returns ready (they are written
    directly), so that train() takes it."""
    e = up._setup(F, C, ODT, SCALE, SEED, max_groups=max_groups)
    e.sink.count.fill_(pp.T_SLOTS)
    e.sink.returns_ready = True
    return e


def _state(e):
    ln = e.learner
    return [t.detach().clone() for t in list(ln._params) + [ln.m, ln.v, ln.step, ln._w2t, ln.stats_t, ln.grad_flat]
            + list(e.seat._w)]


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _host_idx(seed, epoch, count, granule):
    from gym_comm_amd import _lib
    L = _lib.load(lib="policy")
    out = np.zeros(count // granule, np.int32)
    assert L.oc_policy_ppo_perm_host(seed, epoch, count // granule, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return tr.expand(out, granule)


def _twin_epochs(e, epochs, batch_size, granule, seed, first_epoch=0):
    """The EXISTING update() over the numpy-restated indices; returns each minibatch's stats()."""
    per = []
    for ep in range(first_epoch, first_epoch + epochs):
        idx = tr.expand(tr.perm(seed, ep, TOTAL // granule)[0], granule)
        for o, b in tr.cuts(TOTAL, batch_size):
            e.learner.update(e.sink, torch.from_numpy(idx[o:o + b].copy()).cuda())
            per.append(e.learner.stats())
    return per


# ---- the shuffle kernel alone ----------------------------------------------------------------------
@pytest.mark.parametrize("count,granule", [(2, 1), (64, 1), (210, 1), (4097, 1), (210, 10), (210, 35)])
def test_shuffle_kernel_equals_the_host_permutation(count, granule):
    from gym_comm_amd import _lib
    L = _lib.load(lib="policy")
    dev = torch.cuda.current_device()
    values, hyper = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
    ctl = torch.zeros(_lib.PPO_CTL["words"], dtype=torch.int32, device="cuda")
    acc = torch.zeros(_lib.PPO_ACC["words"], dtype=torch.float64, device="cuda")
    t = _lib.PpoTrain(values.data_ptr(), hyper.data_ptr(), ctl.data_ptr(), acc.data_ptr())
    idx = torch.full((count + 64,), -7, dtype=torch.int32, device="cuda")
    for epoch in (0, 1):                                    # two calls: consecutive epochs
        _lib.call(L, "oc_policy_ppo_epoch_begin", dev, ctypes.byref(t), idx.data_ptr(), count, granule, SHUFFLE_SEED)
        got = idx.cpu().numpy()
        assert np.array_equal(got[:count], _host_idx(SHUFFLE_SEED, epoch, count, granule)), epoch
        assert (got[count:] == -7).all()                    # nothing past the end
    words = ctl.cpu().tolist()
    assert words[_lib.PPO_CTL["error"]] == 0 and words[_lib.PPO_CTL["epoch"]] == 2 and words[_lib.PPO_CTL["stop"]] == 0
    # a stopped sequence: nothing is written, the counter stays
    ctl[_lib.PPO_CTL["stop"]] = 1
    idx.fill_(-7)
    _lib.call(L, "oc_policy_ppo_epoch_begin", dev, ctypes.byref(t), idx.data_ptr(), count, granule, SHUFFLE_SEED)
    assert (idx.cpu().numpy() == -7).all() and ctl.cpu().tolist()[_lib.PPO_CTL["epoch"]] == 2


# ---- parity with the existing update ---------------------------------------------------------------
def test_device_train_and_its_graph_are_the_existing_update_bit_for_bit():
    from gym_comm_amd import _lib
    assert [b for _, b in tr.cuts(TOTAL, 64)] == [64, 64, 64, 18]
    a, twin, g = _env(), _env(), _env()
    a.learner.train(a.sink, n_epochs=2, batch_size=64, granule=10, shuffle="device", seed=SHUFFLE_SEED)
    _twin_epochs(twin, 2, 64, 10, SHUFFLE_SEED)
    graph = g.learner.train_graph(g.sink, 2, batch_size=64, granule=10, seed=SHUFFLE_SEED)
    assert int(g.learner.step.item()) == 0                  # the warm-up was undone, the capture ran nothing
    graph.replay()
    torch.cuda.synchronize()
    first = a.learner._idx.clone()
    assert int(a.learner.step.item()) == 8
    assert _same(_state(a), _state(twin)), "train(shuffle='device') against update() over the restated indices"
    assert _same(_state(a), _state(g)), "one replay against the eager sequence"
    assert torch.equal(a.learner._idx, g.learner._idx)
    assert np.array_equal(first.cpu().numpy(), tr.expand(tr.perm(SHUFFLE_SEED, 1, 21)[0], 10))
    # a second train: the epoch counter went on
    a.learner.train(a.sink, n_epochs=2, batch_size=64, granule=10, shuffle="device", seed=SHUFFLE_SEED)
    graph.replay()
    _twin_epochs(twin, 2, 64, 10, SHUFFLE_SEED, first_epoch=2)
    torch.cuda.synchronize()
    assert int(a.learner.step.item()) == 16
    assert _same(_state(a), _state(g)) and _same(_state(a), _state(twin))
    assert not torch.equal(a.learner._idx, first) and torch.equal(a.learner._idx, g.learner._idx)
    for e in (a, g):
        words = e.learner.ctl.cpu().tolist()
        assert words[_lib.PPO_CTL["epoch"]] == 4 and words[_lib.PPO_CTL["error"]] == 0
        st = e.learner.train_stats()
        assert st["updates"] == 8 and st["epochs"] == 2 and not st["stopped"]


# ---- value clipping ----------------------------------------------------------------------------------
def _split(ln):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in ln.grads.items()}


def test_value_clipping_within_the_derived_bounds_and_switched_by_a_device_write():
    inp = tr.vclip_inputs()
    c, hp = inp["c"], pp.test_hp()
    e = _env(max_groups=inp["mg"])
    old_v = e.sink.values.cpu().numpy().reshape(-1)[inp["idx"]]          # what the kernel reads
    case = pp.make_case(e.buf, inp["idx"], e.old_lp)
    ref, rstats, info = tr.vclip_reference(case, old_v, c, hp, e.learner.plan(TOTAL))
    print("clip_range_vf %.6f: %d of %d gates open, margin %.3e, recorded values within %.2e of the emulation's"
          % (c, info["gate"].sum(), TOTAL, info["margin"], np.abs(old_v - inp["old_v"]).max()))
    assert info["margin"] > 0 and 40 < info["gate"].sum() < 170
    e.learner.set_clip_range_vf(c)
    graph = e.learner.train_graph(e.sink, 1, batch_size=None, granule=1, seed=tr.VSEED)
    start = [t.clone() for t in e.learner._train_tensors()]
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(e.learner._idx.cpu().numpy(), inp["idx"])
    stats, got = e.learner.stats(), _split(e.learner)
    clipped_bits = _bits(e.learner.grad_flat).clone()
    worst = pp.clipped_excess(got, stats["grad_norm"], ref, info["bound"], hp)
    for k in pp.NAMES:
        print(k, "excess over the bound %.3e at kernel %.9e reference %.9e bound %.3e" % worst[k])
    for k in pp.STATS:
        tol = info["stat_bound"][k] + 2 * pp.U * abs(rstats[k])
        print(k, "kernel %.9g reference %.9g bound %.3e" % (stats[k], rstats[k], tol))
    for k in pp.NAMES:
        assert worst[k][0] <= 0, (k, worst[k])
    for k in pp.STATS:
        assert abs(stats[k] - rstats[k]) <= info["stat_bound"][k] + 2 * pp.U * abs(rstats[k]), k
    # the unclipped loss is outside the bound here (the CPU tests' `ignored` mutant, on the kernel's side)
    plain, pstats, _ = pp.loss_and_grad(case, hp)
    assert abs(stats["value_loss"] - pstats["value_loss"]) > info["stat_bound"]["value_loss"]
    # eager gives the captured sequence's bits
    twin = _env(max_groups=inp["mg"])
    twin.learner.set_clip_range_vf(c)
    twin.learner.train(twin.sink, n_epochs=1, granule=1, shuffle="device", seed=tr.VSEED)
    assert _same(_state(e), _state(twin))
    # clipping switched off by a device write, the SAME graph: the existing update's bits
    with torch.no_grad():
        for t, s in zip(e.learner._train_tensors(), start):
            t.copy_(s)
    e.learner.set_clip_range_vf(None)
    graph.replay()
    off = _env(max_groups=inp["mg"])
    off.learner.update(off.sink, torch.from_numpy(inp["idx"].copy()).cuda())
    torch.cuda.synchronize()
    assert _same(_state(e), _state(off))
    assert not torch.equal(_bits(e.learner.grad_flat), clipped_bits)


# ---- the KL stop and the accumulated statistics ----------------------------------------------------
_kl = {}


def _one_epoch():
    """One epoch of 64, 64, 64, 18 by the existing update(): its state, and each minibatch's stats()."""
    if not _kl:
        twin = _env()
        per = _twin_epochs(twin, 1, 64, 1, SHUFFLE_SEED)
        kl = [np.float64(np.float32(s["approx_kl"])) for s in per]
        m = np.float64(0.0)
        for v in kl:
            m += v
        _kl.update(state=_state(twin), per=per, mean=float(m / np.float64(len(kl))))
        print("approx_kl per minibatch", kl, "mean", _kl["mean"])
    return _kl


@pytest.mark.parametrize("captured", [False, True])
def test_kl_rule_stops_after_the_epoch_whose_mean_exceeds_the_target(captured):
    ref = _one_epoch()
    m = ref["mean"]
    assert m > 0

    def run(target):
        e = _env()
        e.learner.set_target_kl(target)
        if captured:
            e.learner.train_graph(e.sink, 3, batch_size=64, granule=1, seed=SHUFFLE_SEED).replay()
        else:
            e.learner.train(e.sink, n_epochs=3, batch_size=64, granule=1, shuffle="device", seed=SHUFFLE_SEED)
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
    per = _twin_epochs(twin, 2, 64, 1, SHUFFLE_SEED)
    e.learner.train(e.sink, n_epochs=2, batch_size=64, granule=1, shuffle="device", seed=SHUFFLE_SEED)
    st = e.learner.train_stats()
    print(st)
    assert st["updates"] == len(per) == 8 and st["epochs"] == 2 and not st["stopped"]
    for k in tr.TRAIN_STATS:
        terms = np.array([np.float64(np.float32(s[k])) for s in per])
        want = terms.mean()
        print(k, "train_stats %.12g mean of stats() %.12g" % (st[k], want))
        assert abs(st[k] - want) <= 2 * pp.U * np.abs(terms).mean(), k


# ---- a halted sequence leaves no trace ---------------------------------------------------------------
@pytest.mark.parametrize("word", ["stop", "error"])
def test_a_halted_train_step_writes_nothing(word):
    from gym_comm_amd import _lib
    e = _env()
    ln = e.learner
    ln.lp_out = torch.full((64,), 7.0, device="cuda")
    ln.v_out = torch.full((64,), 7.0, device="cuda")
    idx = torch.from_numpy(pp.make_indices(64)).cuda()
    ln.update(e.sink, idx)                                  # real numbers everywhere, the scratch allocated
    ln.ctl[_lib.PPO_CTL[word]] = 1
    ln.acc.fill_(3.0)
    ln.stats_t.fill_(5.0)
    ln.lp_out.fill_(7.0)
    watched = lambda: _state(e) + [ln._scratch.clone(), ln._train_words.clone(), ln.lp_out.clone(), ln.v_out.clone()]  # noqa: E731
    before = watched()
    _lib.call(ln._L, "oc_policy_ppo_train_step", ln._dev, ctypes.byref(ln._cfg(e.sink, 64)),
              ctypes.byref(ln._train_state(e.sink)), idx.data_ptr(), 64)
    torch.cuda.synchronize()
    assert _same(before, watched())
    ln.ctl[_lib.PPO_CTL[word]] = 0                          # and it was the word that held it back
    _lib.call(ln._L, "oc_policy_ppo_train_step", ln._dev, ctypes.byref(ln._cfg(e.sink, 64)),
              ctypes.byref(ln._train_state(e.sink)), idx.data_ptr(), 64)
    torch.cuda.synchronize()
    assert int(ln.step.item()) == 2 and not _same(before, watched())
