"""The recurrent PPO update (include/oc_policy.h, last section: oc_policy_rppo_*) without a GPU: the float64
reference against torch autograd of the module, the mutants, the exports / struct / prototypes against the
header, the argument checks, the plan by hand, the backward image's packer index by index, the new
translation unit's code object, and the seat's ``set_state`` with both tuple lengths."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import policy_ref as pr  # noqa: E402
import recurrent_ppo_ref as rp  # noqa: E402

ROOT = os.path.dirname(HERE)
FP = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib.load(lib="policy")


def _torch_grads(case, hp):
    """The header's loss through the module in float64 and torch autograd: ({name: grad}, loss)."""
    pol = case["pol"].double()
    for p in pol.parameters():
        p.grad = None
    envs = torch.from_numpy(np.asarray(case["envs"], np.int64))
    T = case["T"]
    E = envs.numel()

    class Obs(dict):
        pass
    h = torch.from_numpy(case["h0"].astype(np.float64))[:, envs].T.contiguous()
    c = torch.from_numpy(case["c0"].astype(np.float64))[:, envs].T.contiguous()
    lps, vals, ents = [], [], []
    for t in range(T):
        obs = Obs()
        obs.rows = torch.from_numpy(case["obs"][t].astype(np.float64))[:, envs]
        obs.timestep = torch.from_numpy(case["ts"][t])[envs]
        mv, cm, (h, c), val = pol(obs, (h, c), torch.from_numpy(case["es"][t])[envs])
        a = torch.from_numpy(case["actions"][t].astype(np.int64))[:, envs]
        lmv, lcm = torch.log_softmax(mv, 0), torch.log_softmax(cm, 0)
        lps.append(lmv.gather(0, a[0:1]).squeeze(0) + lcm.gather(0, a[1:2]).squeeze(0))
        ents.append(-(lmv.exp() * lmv).sum(0) - (lcm.exp() * lcm).sum(0))
        vals.append(val)
    lp, val, ent = torch.stack(lps).reshape(-1), torch.stack(vals).reshape(-1), torch.stack(ents).reshape(-1)
    g = lambda k: torch.from_numpy(case[k].astype(np.float64))[:, envs].reshape(-1)  # noqa: E731
    adv, ret, old = g("adv"), g("ret"), g("old_lp")
    ahat = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old)
    pl = -torch.min(ahat * ratio, ahat * torch.clamp(ratio, 1 - hp.clip, 1 + hp.clip)).mean()
    loss = pl + hp.ent * (-ent.mean()) + hp.vf * ((ret - val) ** 2).mean()
    loss.backward()
    assert lp.numel() == T * E
    grads = {k: getattr(pol, k).grad.numpy().copy() for k in rp.NAMES}
    case["pol"].float()
    return grads, float(loss)


def test_reference_equals_torch_autograd_of_the_module():
    """emulate=False against float64 autograd, T = 6, n = 9, starts at t = 0, mid-sequence and the last step."""
    case = rp.cpu_case()
    assert case["es"][0].any() and case["es"][3].any() and case["es"][5].any() and not case["es"][1].any()
    hp = rp.test_hp()
    want, loss = _torch_grads(case, hp)
    got, stats, _ = rp.loss_and_grad(case, hp, emulate=False)
    assert abs(stats["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    for k in rp.NAMES:
        assert got[k].shape == want[k].shape, k
        scale = np.abs(want[k]).max()
        assert scale > 0 and np.abs(got[k] - want[k]).max() <= 1e-12 * scale, (k, np.abs(got[k] - want[k]).max() / scale)
    # the emulated gradient stays near it at the init scale (fp16 operands), and is not it
    em = rp.loss_and_grad(case, hp, emulate=True)[0]
    d = rp.rel_diff(em, got)
    assert 0 < max(d.values()) < 0.2, d


def test_every_mutant_moves_the_emulated_gradient():
    hp = rp.test_hp()
    cases = [("cpu", rp.cpu_case())] + rp.gpu_cases()
    moves = {name: rp.mutant_moves(case, hp) for name, case in cases}
    for name, mv in moves.items():
        print(name, {m: "%.3g" % v for m, v in mv.items()})
    # a mutant APPLIES to a case when it moves some tensor there at all (case a has one step: nothing recurs)
    applied = {m: [moves[name][m] for name, _ in cases if moves[name][m] > 0] for m in rp.MUTANTS}
    for m in rp.MUTANTS:
        assert applied[m], m
        assert moves["c"][m] > 0 or moves["b"][m] > 0 or moves["a"][m] > 0, m      # and to a GPU case
    mut_min = min(min(v) for v in applied.values())
    print("MUT_MIN", mut_min)
    assert mut_min >= rp.MUT_MIN, (mut_min, rp.MUT_MIN)
    assert rp.TOL_G <= rp.MUT_MIN / 20
    # in the T = 6 case the gradient not cut at starts moves gwx by 0.12 of its scale and gwh by 0.39
    case = rp.cpu_case()
    ref = rp.loss_and_grad(case, hp)[0]
    d = rp.rel_diff(rp.loss_and_grad(case, hp, mutate="not cut at starts")[0], ref)
    assert d["wx"] > 0.1 and d["wh"] > 0.3 and d["w2"] == 0, d
    with pytest.raises(ValueError):
        rp.loss_and_grad(case, hp, mutate="nothing")


_EDGE = {}


def _edge(name):
    """tests/recurrent_ppo_ref.py's edge cases, built once and never changed."""
    if not _EDGE:
        _EDGE.update(rp.edge_cases())
    return _EDGE[name]


def test_the_edge_cases_are_what_they_are_for():
    d, e, e48, f, g = (_edge(k) for k in ("d", "e", "e48", "f", "g"))
    assert [(c["T"], c["n"], len(c["envs"]), c["F"], c["C"], c["odt"]) for c in (d, e, e48, f, g)] == [
        (52, 136, 129, 30, 3, "int8"), (3, 40, 33, 31, 2, "int32"), (3, 40, 33, 46, 2, "int32"), (3, 40, 32, 15, 1, "int8"),
        (6, 36, 1, 47, 7, "float32")]
    assert len(set(d["envs"].tolist())) == 128 and d["envs"][-1] == d["envs"][0] and list(d["envs"][:-1]) != sorted(d["envs"][:-1])
    assert len(set(e["envs"].tolist())) == 33 and len(set(f["envs"].tolist())) == 32 and list(g["envs"]) == [7]
    for c, starts in ((d, (0, 1, 2, 17, 51)), (e, (1,)), (e48, (1,)), (f, (2,)), (g, (2,))):
        mine = c["es"][:, c["envs"]]
        assert [t for t in range(c["T"]) if mine[t].any()] == list(starts)
        assert all(0 < mine[t].sum() < len(c["envs"]) or len(c["envs"]) == 1 for t in starts)
        assert c["obs"].dtype == np.dtype(c["odt"])
    # some sequence of d starts at each of t = 0, 1, 2: three consecutive cuts of one carry
    assert (d["es"][:3, d["envs"]].sum(axis=0) == 3).any()
    # the int8 rows beyond t = 0 are not the rows of t = 0
    assert not np.array_equal(d["obs"][1], d["obs"][0]) and not np.array_equal(f["obs"][2], f["obs"][0])


def test_every_mutant_moves_the_edge_cases_twenty_tolerances():
    """d, e, e48 and f: every mutant applies, and the smallest move is at least 20 x the tolerance of that case."""
    hp = rp.test_hp()
    for name in ("d", "e", "e48", "f"):
        mv = rp.mutant_moves(_edge(name), hp)
        tol_g = rp.tolerances(name)[0]
        print(name, {m: "%.3g" % v for m, v in mv.items()}, "smallest %.4g" % min(mv.values()), "tolerance %.3g" % tol_g)
        assert all(v > 0 for v in mv.values()), (name, mv)
        assert min(mv.values()) >= 20 * tol_g, (name, min(mv.values()), tol_g)
    assert rp.tolerances("d") == (rp.TOL_G_LONG, rp.TOL_S_LONG) and rp.tolerances("g") == (rp.TOL_G, rp.TOL_S)
    # the long case's tolerances are 4 x its own measured figures, rounded up, and the short cases' figures lie
    # within TOL_G / TOL_S
    m = rp.MEASURED
    for kind, tol in (("grad", rp.TOL_G_LONG), ("stats", rp.TOL_S_LONG)):
        largest = max(m[kind][k] for k in ("d_0", "d_1", "d_7"))
        assert 4 * largest <= tol <= 1.01 * 4 * largest, (kind, largest, tol)
    assert all(m["grad"][k] <= rp.TOL_G and m["stats"][k] <= rp.TOL_S for k in ("e", "e48", "f", "g"))


def test_reference_equals_torch_autograd_of_the_module_through_52_steps():
    """emulate=False of case d against float64 autograd: the reference itself at T = 52, E = 129, five starts."""
    case = _edge("d")
    hp = rp.test_hp()
    want, loss = _torch_grads(case, hp)
    got, stats, _ = rp.loss_and_grad(case, hp, emulate=False)
    print("loss", stats["loss"], loss)
    assert abs(stats["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    for k in rp.NAMES:
        assert got[k].shape == want[k].shape, k
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max() / scale
        print(k, "%.3g" % err)
        assert scale > 0 and err <= 1e-12, (k, err)


def test_exports_struct_and_prototypes_match_the_header():
    from gym_comm_amd import _lib, learner, vec_env
    L = _policy_lib()
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_policy_rppo_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(k for k in _lib.LIBS["policy"].protos if k.startswith("oc_policy_rppo_"))
    assert sorted(declared) == ["oc_policy_rppo_grad", "oc_policy_rppo_pack_bwd", "oc_policy_rppo_pack_bwd_elems",
                                "oc_policy_rppo_plan", "oc_policy_rppo_update"]
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.oc_policy_abi_version() == 1
    body = re.search(r"typedef struct \{([^}]*)\} oc_rppo_cfg;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert fields == [n for n, _ in _lib.RppoCfg._fields_], fields
    assert ctypes.sizeof(_lib.RppoCfg) == 9 * 8 + 8 + 16 + 19 * 8 + 6 * 4 + 4 + 4 + 2 * 8     # (4 bytes of padding)
    assert vec_env.RecurrentPPOLearner is learner.RecurrentPPOLearner
    assert learner.RecurrentPPOLearner.__module__ == learner.__name__
    assert issubclass(learner.PPOLearner, learner._Learner) and issubclass(learner.RecurrentPPOLearner, learner._Learner)
    # the section is the header's last, and says what is still out of scope
    tail = hdr[hdr.index("the recurrent seat's PPO update"):]
    assert "oc_policy_lstm_ac(" not in tail
    for phrase in ("truncated windows", "target_kl", "marginal-regularisation", "hidden sizes other than 64",
                   "separate critic LSTM", "the cell inside the step kernel", "measured, not a bound"):
        assert phrase in tail, phrase


def test_argument_checks_come_before_any_device_work_and_name_the_function():
    from gym_comm_amd import _lib
    L = _policy_lib()
    some = 0x1000          # never dereferenced: a refused call launches nothing
    names = [n for n, _ in _lib.RppoCfg._fields_]
    ptrs = [n for n, t in _lib.RppoCfg._fields_ if t is ctypes.c_void_p]

    def cfg(**kw):
        base = {k: some for k in ptrs}
        base.update(n=64, T=4, F=29, C=2, obs_type=0, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999,
                    eps=1e-5, max_groups=0, lp_out=None, v_out=None)
        base.update(kw)
        return _lib.RppoCfg(*[base[k] for k in names])

    for fn in ("oc_policy_rppo_grad", "oc_policy_rppo_update"):
        call = lambda c, envs, E: getattr(L, fn)(None if c is None else ctypes.byref(c), envs, E, None)  # noqa: E731,B023
        refused = [(None, some, 8), (cfg(), None, 8), (cfg(), some, 0), (cfg(T=1), some, 1), (cfg(F=0), some, 8),
                   (cfg(F=63), some, 8), (cfg(C=0), some, 8), (cfg(C=17), some, 8), (cfg(T=0), some, 8),
                   (cfg(obs_type=3), some, 8), (cfg(obs_type=-1), some, 8), (cfg(n=0), some, 8),
                   (cfg(n=2 ** 29, T=4), some, 8), (cfg(n=2 ** 25, T=1), some, 8), (cfg(max_groups=-1), some, 8),
                   (cfg(T=2 ** 20, n=64), some, 2 ** 12), (cfg(scratch=some + 4), some, 8)]
        always = ("obs", "timestep", "actions", "log_probs", "advantages", "returns", "episode_starts", "h0", "c0", "gates",
                  "head", "head_bias", "bwd", "grad", "scratch", "stats", "hyper")
        refused += [(cfg(**{k: None}), some, 8) for k in always]
        if fn.endswith("update"):
            refused += [(cfg(**{k: None}), some, 8) for k in ptrs if k not in always and k not in ("lp_out", "v_out")]
        for args in refused:
            assert call(*args) != 0, args[1:]
            assert L.oc_policy_last_error().startswith(fn.encode() + b": "), L.oc_policy_last_error()
        assert call(cfg(C=17), some, 8) != 0 and b"C <= 16" in L.oc_policy_last_error()
        assert call(cfg(F=63), some, 8) != 0 and b"F + 2 <= 64" in L.oc_policy_last_error()
        assert call(cfg(n=2 ** 29), some, 8) != 0 and b"2^31" in L.oc_policy_last_error()
        assert call(cfg(T=1), some, 1) != 0 and b"E T" in L.oc_policy_last_error()
    plan = (ctypes.c_int64 * 8)()
    for args in ((0, 2, 4, 8, 0), (63, 2, 4, 8, 0), (29, 0, 4, 8, 0), (29, 17, 4, 8, 0), (29, 2, 0, 8, 0), (29, 2, 4, 0, 0),
                 (29, 2, 1, 1, 0), (29, 2, 4, 8, -1), (29, 2, 2 ** 20, 2 ** 12, 0)):
        assert L.oc_policy_rppo_plan(*args, plan) != 0, args
        assert L.oc_policy_last_error().startswith(b"oc_policy_rppo_plan: ")
    assert L.oc_policy_rppo_plan(29, 2, 4, 8, 0, None) != 0
    w = np.zeros((256, 64), np.float32)
    out = np.zeros(L.oc_policy_rppo_pack_bwd_elems(), np.float32)
    for args in ((None, FP(w), FP(w), 2, FP(out)), (FP(w), None, FP(w), 2, FP(out)), (FP(w), FP(w), None, 2, FP(out)),
                 (FP(w), FP(w), FP(w), 2, None), (FP(w), FP(w), FP(w), 0, FP(out)), (FP(w), FP(w), FP(w), 17, FP(out))):
        assert L.oc_policy_rppo_pack_bwd(*args) != 0
        assert L.oc_policy_last_error().startswith(b"oc_policy_rppo_pack_bwd: ")


def test_plan_by_hand():
    """plan = (ceil(E / 32), Gw = min(T ceil(E / 32), cap), ceil(T tiles / Gw), P, scratch, ceil(P / 256), 6, 416) with
    scratch = 2 Gr + 416 T E + Gw P + 8 ceil(E / 32) floats and P = 256 (F + 2) + 16384 + 65 (4 + C) + 65."""
    L = _policy_lib()
    plan = (ctypes.c_int64 * 8)()
    P = 256 * 16 + 16384 + 65 * 5 + 65                                       # F = 14, C = 1: 20870
    assert L.oc_policy_rppo_plan(14, 1, 1, 2, 0, plan) == 0
    assert list(plan) == [1, 1, 1, 20870, 2 * 82 + 416 * 2 + 20870 + 8, 82, 6, 416] and P == 20870
    P = 256 * 64 + 16384 + 65 * 20 + 65                                      # F = 62, C = 16: 34133
    assert L.oc_policy_rppo_plan(62, 16, 7, 96, 0, plan) == 0
    assert list(plan) == [3, 21, 1, 34133, 2 * 134 + 416 * 7 * 96 + 21 * 34133 + 24, 134, 6, 416]
    assert L.oc_policy_rppo_plan(62, 16, 7, 96, 4, plan) == 0                # a cap: 21 pairs over 4 workgroups
    assert list(plan)[:3] == [3, 4, 6] and plan[4] == 2 * 134 + 416 * 7 * 96 + 4 * 34133 + 24
    P = 256 * 31 + 16384 + 65 * 6 + 65                                       # F = 29, C = 2: the scratch passes 2^31 floats
    assert L.oc_policy_rppo_plan(29, 2, 128, 65536, 0, plan) == 0
    assert list(plan) == [2048, 256, 1024, P, 2 * 97 + 416 * 128 * 65536 + 256 * P + 8 * 2048, 97, 6, 416]
    assert plan[4] > 2 ** 31


def test_plan_by_hand_of_the_ragged_rounds():
    """The plans tests/test_recurrent_ppo_gpu.py's ragged runs assert: Gw does not divide T tiles, so the last round
    of the weight-gradient kernel has idle workgroups."""
    L = _policy_lib()
    plan = (ctypes.c_int64 * 8)()
    d = _edge("d")
    T, E, F, C = d["T"], len(d["envs"]), d["F"], d["C"]
    assert (T, E, F, C) == (52, 129, 30, 3)
    P = 256 * 32 + 16384 + 65 * 7 + 65                                       # F = 30, C = 3: 25096
    assert L.oc_policy_rppo_plan(F, C, T, E, 0, plan) == 0                   # 260 items over the default cap
    print("d, max_groups 0:", list(plan))
    assert list(plan) == [5, 256, 2, P, 2 * 99 + 416 * 52 * 129 + 256 * P + 40, 99, 6, 416] and P == 25096
    assert 256 * 2 - 52 * 5 == 252                                           # the second round: 4 live items of 256
    assert L.oc_policy_rppo_plan(F, C, T, E, 7, plan) == 0
    print("d, max_groups 7:", list(plan))
    assert list(plan)[:3] == [5, 7, 38] and 7 * 38 == 266 and 52 * 5 == 260
    assert L.oc_policy_rppo_plan(62, 16, 7, 96, 4, plan) == 0                # case c
    print("c, max_groups 4:", list(plan))
    assert list(plan)[:3] == [3, 4, 6] and 4 * 6 == 24 and 7 * 3 == 21


@pytest.mark.parametrize("C", [1, 5, 16])
def test_backward_image_index_by_index(C):
    """bwd = Wh^T [2][8][16][64] then [W2; wv]^T [2][16][64]: the fp16 value of the folded weight times the inverse
    of its fold, one float32 product."""
    L = _policy_lib()
    rng = np.random.default_rng(40 + C)
    wh = rng.uniform(-1, 1, (256, 64)).astype(np.float32)
    w2, wv = rng.uniform(-1, 1, (4 + C, 64)).astype(np.float32), rng.uniform(-1, 1, 64).astype(np.float32)
    n = L.oc_policy_rppo_pack_bwd_elems()
    assert n == 2 * 8 * 16 * 64 + 2 * 16 * 64
    out = np.full(n, np.nan, np.float32)
    assert L.oc_policy_rppo_pack_bwd(FP(wh), FP(w2), FP(wv), C, FP(out)) == 0
    f16 = lambda v: np.float32(np.float16(np.float32(v)))  # noqa: E731
    LN2 = np.float32(0.6931471805599453)
    wht = out[:16384].reshape(2, 8, 16, 64)
    for m in range(2):
        for u in range(8):
            gate = u >> 1
            fold = np.float32(2) * pr.LOG2E32 if gate == 2 else -pr.LOG2E32
            unfold = np.float32(0.5) * LN2 if gate == 2 else -LN2
            for q in range(16):
                for l in range(64):
                    row = 64 * gate + 32 * (u & 1) + (q & 3) + 8 * (q >> 2) + 4 * (l >> 5)
                    want = np.float32(f16(fold * wh[row, 32 * m + (l & 31)]) * unfold)
                    assert wht[m, u, q, l].view(np.uint32) == want.view(np.uint32), (m, u, q, l)
    # ... which is the weight itself to fp16 precision
    assert np.abs(wht[1, 5, 3, 40] - wh[64 * 2 + 32 + 3 + 4, 32 + 8]) < 1e-3
    row_of = {o: w2[o] for o in range(4)}
    for c in range(C):
        row_of[4 + (c & 3) + 8 * (c >> 2)] = w2[4 + c]
    row_of[8] = wv
    w2t = out[16384:].reshape(2, 16, 64)
    for m in range(2):
        for t in range(16):
            for l in range(64):
                w = row_of.get((t & 3) + 8 * (t >> 2) + 4 * (l >> 5))
                want = np.float32(0) if w is None else np.float32(f16(pr.LOG2E32 * w[32 * m + (l & 31)]) * LN2)
                assert w2t[m, t, l].view(np.uint32) == want.view(np.uint32), (m, t, l)


def test_the_new_unit_sits_between_the_seat_and_the_train_sequence_and_uses_no_scratch(tmp_path):
    from gym_comm_amd import build
    rec = build.LIBS["policy"]
    at = rec.sources.index("oc_policy_rppo.hip")
    assert rec.sources.index("oc_policy_lstm.hip") < at < rec.sources.index("oc_policy_train.hip") == len(rec.sources) - 1
    text = open(os.path.join(build.CSRC, "oc_policy_rppo.hip")).read() + open(os.path.join(build.CSRC, "oc_policy_rppo_device.h")).read()
    for inc in re.findall(r'#include "(oc_\w+\.h)"', text):
        assert inc in rec.local_headers, inc
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    co = str(tmp_path / "rppo.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, "oc_policy_rppo.hip"), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    print(list(zip(names, regs, lds)))
    count = lambda part: sum(part in n for n in names)  # noqa: E731
    assert len(names) == 11 and all("k_rppo_" in n for n in names), names
    assert (count("k_rppo_adv"), count("k_rppo_forward"), count("k_rppo_backward"), count("k_rppo_wgrad"),
            count("k_rppo_reduce"), count("k_rppo_finish")) == (1, 3, 1, 3, 1, 2)
    assert len(sizes) == 11 and max(sizes) == 0, sizes
    assert len(regs) == 11 and max(regs) <= 512, regs
    assert len(lds) == 11 and max(lds) <= 160 * 1024, lds


def test_the_seat_accepts_states_of_both_lengths():
    """``set_state`` takes the 7-tuple a seat gave before it kept h0 / c0, and the 9-tuple it gives now (host
    logic: the seat's tensors stand on the CPU here, no launch is made)."""
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic
    n = 6
    seat = FusedRecurrentPartner.__new__(FusedRecurrentPartner)
    seat.sink = None
    seat.policy = LSTMActorCritic(3, 2)
    z = lambda *s: torch.zeros(s)  # noqa: E731
    seat._rng, seat.episode_start, seat.log_prob, seat.value = torch.zeros((2, n), dtype=torch.int32), z(n), z(n), z(n)
    seat.h, seat.c, seat.h0, seat.c0 = z(64, n), z(64, n), z(64, n), z(64, n)
    seat.logits = None
    old = (torch.ones((2, n), dtype=torch.int32), z(n) + 1, z(n) + 2, z(n) + 3, None, z(64, n) + 4, z(64, n) + 5)
    seat.set_state(old)
    assert (seat.h == 4).all() and (seat.c == 5).all() and (seat.h0 == 0).all() and (seat.c0 == 0).all()
    seat.set_state(old + (z(64, n) + 6, z(64, n) + 7))
    assert (seat.h0 == 6).all() and (seat.c0 == 7).all() and (seat._rng == 1).all()
    seat.begin_rollout()                                                     # h -> h0, c -> c0; episode_start stays
    assert (seat.h0 == 4).all() and (seat.c0 == 5).all() and (seat.episode_start == 1).all()
    seat.log_prob = torch.zeros(n)                                           # (get_state's _buffers finds its buffers)
    assert len(seat.get_state(n)) == 9
