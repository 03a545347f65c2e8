"""No GPU: the recurrent learner's train sequence (include/oc_policy.h, last section: oc_policy_recurrent_train_step;
``RecurrentPPOLearner.train(shuffle="device")``, ``train_graph``).  The float64 reference of the value-clipped loss
against torch autograd of the module, its planted bugs on the GPU tests' cases, the surface against the header,
the entry point's argument checks, the cut rule, the new translation unit's code object, and the host logic."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import recurrent_ppo_ref as rp  # noqa: E402
import recurrent_train_ref as rt  # noqa: E402

NAME = b"oc_policy_recurrent_train_step"


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib, _lib.load(lib="policy")


# ---- the value-clipped reference -----------------------------------------------------------------------------------
def _torch_clipped(case, old_v, c, hp):
    """The header's loss with torch.clamp through the module in float64 and torch autograd: ({name: grad}, loss,
    value_loss)."""
    pol = case["pol"].double()
    for p in pol.parameters():
        p.grad = None
    envs = torch.from_numpy(np.asarray(case["envs"], np.int64))
    T = case["T"]

    class Obs(dict):
        pass
    h = torch.from_numpy(case["h0"].astype(np.float64))[:, envs].T.contiguous()
    cc = torch.from_numpy(case["c0"].astype(np.float64))[:, envs].T.contiguous()
    lps, vals, ents = [], [], []
    for t in range(T):
        obs = Obs()
        obs.rows = torch.from_numpy(case["obs"][t].astype(np.float64))[:, envs]
        obs.timestep = torch.from_numpy(case["ts"][t])[envs]
        mv, cm, (h, cc), val = pol(obs, (h, cc), torch.from_numpy(case["es"][t])[envs])
        a = torch.from_numpy(case["actions"][t].astype(np.int64))[:, envs]
        lmv, lcm = torch.log_softmax(mv, 0), torch.log_softmax(cm, 0)
        lps.append(lmv.gather(0, a[0:1]).squeeze(0) + lcm.gather(0, a[1:2]).squeeze(0))
        ents.append(-(lmv.exp() * lmv).sum(0) - (lcm.exp() * lcm).sum(0))
        vals.append(val)
    lp, val, ent = torch.stack(lps).reshape(-1), torch.stack(vals).reshape(-1), torch.stack(ents).reshape(-1)
    g = lambda a: torch.from_numpy(np.asarray(a).astype(np.float64))[:, envs].reshape(-1)  # noqa: E731
    adv, ret, old, oldv = g(case["adv"]), g(case["ret"]), g(case["old_lp"]), g(old_v)
    ahat = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    pl = -torch.min(ahat * ratio, ahat * torch.clamp(ratio, 1 - hp.clip, 1 + hp.clip)).mean()
    vp = oldv + torch.clamp(val - oldv, -c, c)
    vl = ((ret - vp) ** 2).mean()
    loss = pl + hp.ent * (-ent.mean()) + hp.vf * vl
    loss.backward()
    grads = {k: getattr(pol, k).grad.numpy().copy() for k in rp.NAMES}
    case["pol"].float()
    return grads, loss.item(), vl.item()


def test_clipped_reference_equals_torch_autograd_with_clamp():
    """emulate=False against float64 autograd of the module with torch.clamp, T = 6, n = 9."""
    case = rp.cpu_case()
    hp = rp.test_hp()
    old_v = rt.recorded_values(case)
    c = float(np.float32(rt.C_VF))
    got, stats, info = rt.clipped_loss_and_grad(case, old_v, c, hp, emulate=False)
    assert 0 < info["gate"].sum() < info["gate"].size                          # both sides of the clamp occur
    want, loss, vl = _torch_clipped(case, old_v, c, hp)
    assert abs(stats["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(stats["value_loss"] - vl) <= 1e-12 * max(1.0, abs(vl))
    for k in rp.NAMES:
        assert got[k].shape == want[k].shape, k
        scale = np.abs(want[k]).max()
        assert scale > 0 and np.abs(got[k] - want[k]).max() <= 1e-12 * scale, (k, np.abs(got[k] - want[k]).max() / scale)
    # ... and it is not the unclipped loss
    plain = rp.loss_and_grad(case, hp, emulate=False)
    assert abs(plain[1]["value_loss"] - vl) > 1e-3 and max(rp.rel_diff(plain[0], want).values()) > 1e-3


def test_gate_conditions_and_every_value_clipping_mutant_moves_the_emulated_gradient():
    hp = rp.test_hp()
    smallest = np.inf
    for name, case in rp.gpu_cases()[1:]:                                      # b and c
        old_v = rt.recorded_values(case)
        share, margin = rt.gate_conditions(case, old_v, rt.C_VF)
        print("case %s: open gates %.3f, min | |v - old_v| - c | %.4f" % (name, share, margin))
        assert 0.3 <= share <= 0.7 and margin > 0.05
        moves = rt.vclip_moves(case, old_v, rt.C_VF, hp)
        print("case", name, {m: "%.3g" % v for m, v in moves.items()})
        smallest = min(smallest, min(moves.values()))
    print("smallest move %.4g (20 x TOL_G = %.4g)" % (smallest, 20 * rp.TOL_G))
    assert smallest >= 20 * rp.TOL_G
    with pytest.raises(ValueError):
        rt.clipped_loss_and_grad(rp.cpu_case(), rt.recorded_values(rp.cpu_case()), rt.C_VF, hp, mutate="nothing")


# ---- the surface -----------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    _l, L = _policy_lib()
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    m = re.search(r"OC_API\s+int\s+oc_policy_recurrent_train_step\s*\(([^)]*)\)", hdr)
    assert m, "the header declares oc_policy_recurrent_train_step"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const oc_rppo_cfg *cfg", "const oc_ppo_train *train", "const int32_t *envs", "int32_t E", "void *stream"]
    proto = _l.LIBS["policy"].protos["oc_policy_recurrent_train_step"]
    P, vp, i32 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int32
    assert proto[0] is ctypes.c_int and len(proto[1]) == 5
    assert proto[1][0]._type_ is _l.RppoCfg and proto[1][1]._type_ is _l.PpoTrain and proto[1][2:] == [vp, i32, vp]
    assert P(_l.RppoCfg) is proto[1][0]
    assert getattr(L, "oc_policy_recurrent_train_step") is not None and L.oc_policy_abi_version() == 1
    # the recurrent update's OUT OF SCOPE list no longer names the train sequence; the others stay
    upd = hdr[hdr.index("the recurrent seat's PPO update"):hdr.index("the recurrent learner's train()")]
    scope = upd[upd.index("OUT OF SCOPE"):upd.index("Sequences.")]
    assert "train sequence" not in scope and "train_graph" not in scope and "target_kl" not in scope
    for phrase in ("truncated windows", "marginal-regularisation", "hidden sizes other than 64", "separate critic LSTM",
                   "the cell inside the step kernel"):
        assert phrase in scope, phrase
    # the new section is the header's last, names its KL rule and says whose it is not
    last = hdr[hdr.index("the recurrent learner's train()"):]
    assert last.index("oc_policy_recurrent_train_step") > 0 and "OC_API" in last and "oc_policy_lstm_ac(" not in last
    assert hdr.rindex("/* ----") == hdr.index("/* ---- the recurrent learner's train()")
    flat = " ".join(last.split())
    for phrase in ("learn.py:328-332", "END of an epoch", "NOT sb3_contrib RecurrentPPO's", "mid-epoch",
                   "ppo_recurrent.py:407-412", "OUT OF SCOPE: sb3_contrib's mid-epoch break", "target_kl",
                   "truncated windows", "marginal-regularisation"):
        assert phrase in flat, phrase


def test_argument_checks_come_before_any_device_work_and_name_the_function():
    _l, L = _policy_lib()
    some = 0x1000          # never dereferenced: a refused call launches nothing
    names = [n for n, _ in _l.RppoCfg._fields_]
    ptrs = [n for n, t in _l.RppoCfg._fields_ if t is ctypes.c_void_p]

    def cfg(**kw):
        base = {k: some for k in ptrs}
        base.update(n=64, T=4, F=29, C=2, obs_type=0, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999,
                    eps=1e-5, max_groups=0, lp_out=None, v_out=None)
        base.update(kw)
        return _l.RppoCfg(*[base[k] for k in names])

    def train(**kw):
        t = _l.PpoTrain(some, some, some, some)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def refused(c, t, envs, E, text):
        rc = L.oc_policy_recurrent_train_step(None if c is None else ctypes.byref(c), None if t is None else ctypes.byref(t),
                                              envs, E, None)
        err = L.oc_policy_last_error()
        assert rc != 0 and err.startswith(NAME + b": ") and text in err, (rc, err, text)

    refused(None, train(), some, 8, b"cfg")
    refused(cfg(), None, some, 8, b"train")
    refused(cfg(), train(), None, 8, b"envs")
    for field in ("values", "hyper_ext", "ctl", "acc"):
        refused(cfg(), train(**{field: None}), some, 8, b"NULL")
    refused(cfg(), train(), some, 0, b"E >= 1")
    refused(cfg(T=1), train(), some, 1, b"E T")
    refused(cfg(C=17), train(), some, 8, b"C <= 16")
    refused(cfg(F=63), train(), some, 8, b"F + 2 <= 64")
    refused(cfg(scratch=some + 4), train(), some, 8, b"8-byte aligned")
    for k in ("p_wx", "p_wt", "p_b", "p_wh", "p_w2", "p_b2", "p_wv", "p_bv", "m", "v", "step"):
        refused(cfg(**{k: None}), train(), some, 8, b"master weights")
    for k in ("obs", "episode_starts", "h0", "bwd", "stats", "hyper"):
        refused(cfg(**{k: None}), train(), some, 8, b"NULL")
    refused(cfg(n=2 ** 29), train(), some, 8, b"2^31")
    refused(cfg(obs_type=3), train(), some, 8, b"obs_type")
    assert not NAME.startswith(b"oc_policy_rppo_") and not NAME.startswith(b"oc_policy_lstm_")


def test_the_cuts_are_minibatches_sizes():
    from gym_comm_amd import learner
    for n, T, per, want in ((100, 7, 32, [32, 32, 32, 4]), (100, 7, None, [100]), (100, 7, 99, [99, 1]), (33, 1, 32, [32])):
        assert [E for _, E in learner.env_cuts(n, T, per)] == want
        assert [o for o, _ in learner.env_cuts(n, T, per)] == [i * (per or n) for i in range(len(want))]
        assert learner.env_cuts(n, T, per) == rt.env_cuts(n, T, per)
        split = torch.arange(n).split(int(per or n))                           # what ``minibatches`` does
        assert [b.numel() for b in split if b.numel() * T >= 2] == want
    with pytest.raises(ValueError):
        learner.env_cuts(100, 7, -1)


# ---- the code object -----------------------------------------------------------------------------------------------
def test_the_new_unit_holds_the_ten_train_kernels_and_uses_no_scratch(tmp_path):
    from gym_comm_amd import build
    rec = build.LIBS["policy"]
    at = rec.sources.index("oc_policy_rtrain.hip")
    assert rec.sources.index("oc_policy_rppo.hip") == at - 1 and rec.sources.index("oc_policy_train.hip") == at + 1
    assert rec.sources[-1] == "oc_policy_train.hip"
    seen, todo = set(), ["oc_policy_rtrain.hip"]
    while todo:                                                                # every local include, transitively
        name = todo.pop()
        for inc in re.findall(r'#include "(oc_\w+\.h)"', open(os.path.join(build.CSRC, name)).read()):
            assert inc in rec.local_headers, inc
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert "oc_policy_rppo_host.h" in seen and "oc_policy_rppo_device.h" in seen
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    co = str(tmp_path / "rtrain.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, "oc_policy_rtrain.hip"), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    print(list(zip(names, regs, lds)))
    count = lambda part: sum(part in n for n in names)  # noqa: E731
    assert len(names) == 10 and all("k_rppo_" in n for n in names), names
    assert (count("k_rppo_adv"), count("k_rppo_forward"), count("k_rppo_backward"), count("k_rppo_wgrad"),
            count("k_rppo_reduce"), count("k_rppo_finish")) == (1, 3, 1, 3, 1, 1)
    assert len(sizes) == 10 and max(sizes) == 0, sizes
    assert len(regs) == 10 and max(regs) <= 512, regs
    assert len(lds) == 10 and max(lds) <= 160 * 1024, lds


# ---- host logic ----------------------------------------------------------------------------------------------------
def test_host_logic_without_a_gpu():
    from gym_comm_amd import learner
    R, M = learner.RecurrentPPOLearner, learner.PPOLearner
    with pytest.raises(ValueError, match="shuffle"):
        R.__new__(R).train(None, shuffle="nonsense")                           # refused before the sink is looked at
    params = list(inspect.signature(R.train).parameters)
    assert params == ["self", "sink", "n_epochs", "envs_per_batch", "granule", "generator", "shuffle", "seed"]
    sig = inspect.signature(R.train).parameters
    assert sig["shuffle"].default == "torch" and sig["seed"].default == 0
    assert list(inspect.signature(R.train_graph).parameters) == ["self", "sink", "n_epochs", "envs_per_batch", "granule", "seed"]
    init = inspect.signature(R.__init__).parameters
    assert list(init)[-2:] == ["clip_range_vf", "target_kl"] and init["clip_range_vf"].default is None
    assert "replay only on a full" in " ".join(R.train_graph.__doc__.split())
    # one copy of the train sequence's state and readers, for both learners
    for name in ("set_clip_range_vf", "set_target_kl", "_train_state", "train_stats", "set_lr", "set_clip_range"):
        assert getattr(R, name) is getattr(M, name) is getattr(learner._Learner, name), name
    for name in ("train", "train_graph", "_train_tensors", "_sequence", "minibatches", "update", "grad", "refresh", "plan"):
        assert name in vars(R) and name in vars(M), name
    assert list(inspect.signature(M.train).parameters) == ["self", "sink", "n_epochs", "batch_size", "granule", "generator",
                                                           "shuffle", "seed"]
    assert list(inspect.signature(M.train_graph).parameters) == ["self", "sink", "n_epochs", "batch_size", "granule", "seed"]
    # the attributes the MLP learner's tests reach into are set by the shared initialiser
    src = inspect.getsource(learner._Learner._init_train_state)
    for attr in ("hyper_ext", "_train_words", "acc", "ctl", "_idx", "_trains"):
        assert "self." + attr in src, attr
    assert "_init_train_state" in inspect.getsource(M.__init__) and "_init_train_state" in inspect.getsource(R.__init__)
