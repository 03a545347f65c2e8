"""The host side of the recurrent seat (include/oc_policy.h, last section: oc_policy_lstm_ac) without a GPU:
the three packers index by index against the header's layout sentences, the argument checks, the exports,
the module (parameters, draw rule, torch.nn.LSTMCell), the float64 reference against the module, the
sampling case's seed, and the new translation unit's code object."""
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
import recurrent_ref as rr  # noqa: E402

ROOT = os.path.dirname(HERE)
FP = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
VP = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
SHAPES = [(7, 1), (29, 2), (46, 5), (62, 16)]          # 1, 2, 3, 4 k-steps over x


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib.load(lib="policy")


def _h16(v):
    return np.float16(np.float32(v)).view(np.uint16)


@pytest.mark.parametrize("F,C", SHAPES)
def test_packers_index_by_index(F, C):
    """gates [4][2][ks][64][8]: element j of lane l, tile (gate, m), k-step s is the folded [Wx | wt | b | 0][64 gate +
    32 m + (l & 31)][16 s + 8 (l >> 5) + j] for an x k-step and the folded Wh[same row][16 s' + 8 (j >> 2) +
    4 (l >> 5) + (j & 3)] for the s'-th k-step over h; the fold is -log2(e), 2 log2(e) for gate g, the
    product in fp32, rounded once.  head / head_bias: pack_w2v's / pack_b2v's maps holding log2(e) [W2; wv]
    and log2(e) [b2; bv]."""
    L = _policy_lib()
    rng = np.random.default_rng(10 * F + C)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    kx = (F + 2 + 15) // 16
    ks = L.oc_policy_lstm_ksteps(F)
    assert ks == kx + 4 == L.oc_policy_ksteps(F) + 4 and kx == SHAPES.index((F, C)) + 1
    for scale in (1.0, 8.0):
        wx, wt, b = f32(rng.uniform(-1, 1, (256, F)) * scale), f32(rng.uniform(-1, 1, 256) * scale), f32(rng.uniform(-1, 1, 256) * scale)
        wh = f32(rng.uniform(-1, 1, (256, 64)) * scale / 8)
        w2, b2 = f32(rng.uniform(-1, 1, (4 + C, 64)) * scale / 8), f32(rng.uniform(-1, 1, 4 + C) * scale)
        wv, bv = f32(rng.uniform(-1, 1, 64) * scale / 8), f32(rng.uniform(-1, 1, 1) * scale)
        og = np.full((4, 2, ks, 64, 8), 0xFFFF, np.uint16)
        oh, ob = np.full((4, 64, 8), 0xFFFF, np.uint16), np.full((64, 16), np.nan, np.float32)
        assert L.oc_policy_lstm_pack_gates(FP(wx), FP(wt), FP(b), FP(wh), F, VP(og)) == 0
        assert L.oc_policy_lstm_pack_head(FP(w2), FP(wv), C, VP(oh)) == 0
        assert L.oc_policy_lstm_pack_head_bias(FP(b2), FP(bv), C, FP(ob)) == 0
        aug = np.concatenate([wx, wt.reshape(-1, 1), b.reshape(-1, 1)], axis=1)
        for gate in range(4):
            fold = np.float32(2) * pr.LOG2E32 if gate == 2 else -pr.LOG2E32
            for m in range(2):
                for s in range(ks):
                    for l in range(64):
                        row = 64 * gate + 32 * m + (l & 31)
                        for j in range(8):
                            if s < kx:
                                k = 16 * s + 8 * (l >> 5) + j
                                v = aug[row, k] if k < F + 2 else np.float32(0)
                            else:
                                v = wh[row, 16 * (s - kx) + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)]
                            assert og[gate, m, s, l, j] == _h16(fold * v), (gate, m, s, l, j)
        # the reference folds the same values (it shares no code with the packer)
        A = rr.fold_gates(wx, wt, b, wh)
        assert A.shape == (256, F + 2 + 64) and _h16(A[70, 3]) == og[1, 0, 0, 6, 3] and _h16(A[200, F + 2 + 21]) == og[3, 0, kx + 1, 40, 1]
        row_of = {o: w2[o] for o in range(4)}
        bias_of = {o: b2[o] for o in range(4)}
        for c in range(C):
            row_of[4 + (c & 3) + 8 * (c >> 2)], bias_of[4 + (c & 3) + 8 * (c >> 2)] = w2[4 + c], b2[4 + c]
        assert 8 not in row_of
        row_of[8], bias_of[8] = wv, bv[0]
        for s in range(4):
            for l in range(64):
                for j in range(8):
                    w = row_of.get(l & 31)
                    want = 0 if w is None else _h16(pr.LOG2E32 * w[16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)])
                    assert oh[s, l, j] == want, (s, l, j)
        for l in range(64):
            for q in range(16):
                bias = bias_of.get((q & 3) + 8 * (q >> 2) + 4 * (l >> 5))
                want = np.float32(0) if bias is None else np.float32(pr.LOG2E32 * np.float32(bias))
                assert ob[l, q].view(np.uint32) == want.view(np.uint32), (l, q)
        Wh16, hb = rr.fold_head(w2, wv, b2, bv)
        assert _h16(Wh16[-1, 5]) == oh[0, 40, 1] and np.float32(hb[-1]).view(np.uint32) == ob[0, 4].view(np.uint32)


def test_argument_checks_come_before_any_device_work_and_name_the_function():
    from gym_comm_amd import _lib
    L = _policy_lib()
    some = 0x1000          # never dereferenced: a refused call launches nothing
    names = [n for n, _ in _lib.PolicyLstmPlayer._fields_]

    def player(**kw):
        base = {k: some for k in ("obs", "gates", "head", "head_bias", "h_in", "c_in")}
        base.update(kw)
        return _lib.PolicyLstmPlayer(*[base.get(k) for k in names])

    call = lambda pl, ts, F, C, ot, n: L.oc_policy_lstm_ac(None if pl is None else ctypes.byref(pl), ts, F, C, ot, n, None)  # noqa: E731
    good = player()
    refused = [(good, some, 29, 17, 0, 64), (good, some, 63, 2, 0, 64), (good, some, 0, 2, 0, 64), (good, some, 29, 0, 0, 64),
               (good, some, 29, 2, 3, 64), (good, some, 29, 2, -1, 64), (good, some, 29, 2, 0, -1), (good, None, 29, 2, 0, 64),
               (None, some, 29, 2, 0, 64), (good, some, 29, 2, 0, 2 ** 25)]
    refused += [(player(**{k: None}), some, 29, 2, 0, 64) for k in ("obs", "gates", "head", "head_bias", "h_in", "c_in")]
    refused += [(player(move_row=some), some, 29, 2, 0, 64), (player(comm_row=some), some, 29, 2, 0, 64)]
    for args in refused:
        assert call(*args) != 0, args[1:]
        assert L.oc_policy_last_error().startswith(b"oc_policy_lstm_ac: "), L.oc_policy_last_error()
    assert call(good, some, 29, 17, 0, 64) != 0 and b"C <= 16" in L.oc_policy_last_error()
    assert call(good, some, 63, 2, 0, 64) != 0 and b"F + 2 <= 64" in L.oc_policy_last_error()
    assert call(player(move_row=some), some, 29, 2, 0, 64) != 0 and b"together" in L.oc_policy_last_error()
    assert call(good, some, 29, 2, 0, 2 ** 25) != 0 and b"2^31" in L.oc_policy_last_error()
    assert call(good, some, 62, 16, 2, 0) == 0               # n == 0: nothing to do
    w = np.zeros((256, 64), np.float32)
    og, ob = np.zeros((4, 2, 8, 64, 8), np.uint16), np.zeros((64, 16), np.float32)
    v = np.zeros(256, np.float32)
    for fn, args in (("oc_policy_lstm_pack_gates", (FP(w), FP(v), FP(v), FP(w), 63, VP(og))),
                     ("oc_policy_lstm_pack_gates", (FP(w), None, FP(v), FP(w), 29, VP(og))),
                     ("oc_policy_lstm_pack_head", (FP(w), FP(v), 17, VP(og))),
                     ("oc_policy_lstm_pack_head", (FP(w), None, 2, VP(og))),
                     ("oc_policy_lstm_pack_head_bias", (FP(v), FP(v), 0, FP(ob))),
                     ("oc_policy_lstm_pack_head_bias", (None, FP(v), 2, FP(ob)))):
        assert getattr(L, fn)(*args) != 0 and L.oc_policy_last_error().startswith(fn.encode() + b": "), fn


def test_exports_and_the_player_struct_match_the_header():
    from gym_comm_amd import _lib, vec_env, partners
    L = _policy_lib()
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_policy_lstm_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(k for k in _lib.LIBS["policy"].protos if k.startswith("oc_policy_lstm_"))
    assert sorted(declared) == ["oc_policy_lstm_ac", "oc_policy_lstm_ksteps", "oc_policy_lstm_pack_gates",
                                "oc_policy_lstm_pack_head", "oc_policy_lstm_pack_head_bias"]
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.oc_policy_abi_version() == 1
    body = re.search(r"typedef struct \{([^}]*)\} oc_policy_lstm_player;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*\s*(\w+)", decl)]
    assert fields == [n for n, _ in _lib.PolicyLstmPlayer._fields_] and len(fields) == 17
    for name in ("LSTMActorCritic", "FusedRecurrentPartner"):
        assert getattr(vec_env, name) is getattr(partners, name) and getattr(partners, name).__module__ == partners.__name__


def test_module_parameters_draw_rule_and_lstm_cell():
    from gym_comm_amd.vec_env import LSTMActorCritic, MLPPolicy
    S, C, n = 5, 3, 40
    F = 22 + S + 2 * C
    pol = LSTMActorCritic(S, C, seed=11)
    shapes = [("wx", (256, F)), ("wt", (256, 1)), ("b", (256, 1)), ("wh", (256, 64)), ("w2", (4 + C, 64)), ("b2", (4 + C, 1)),
              ("wv", (1, 64)), ("bv", (1, 1))]
    assert [(k, tuple(t.shape)) for k, t in pol.named_parameters()] == shapes
    g = torch.Generator().manual_seed(11)          # MLPPolicy's rule: uniform in +-1/sqrt(fan-in), one generator
    for k, t in pol.named_parameters():
        want = (torch.rand(t.shape, generator=g) * 2 - 1) / float(np.sqrt(t.shape[-1]))
        assert torch.equal(t.detach(), want), k
    assert pol.feature_major and MLPPolicy.feature_major
    assert not torch.equal(pol.wx, LSTMActorCritic(S, C, seed=12).wx)

    class Obs(dict):
        pass
    gen = torch.Generator().manual_seed(3)
    obs = Obs()
    obs.rows, obs.timestep = torch.randn((F, n), generator=gen), torch.rand(n, generator=gen, dtype=torch.float64)
    state = (torch.randn((n, 64), generator=gen), torch.randn((n, 64), generator=gen))
    es = (torch.rand(n, generator=gen) < 0.4).float()
    state[0][0, 0], state[1][0, 1], es[0] = float("nan"), float("inf"), 1.0       # a starting env: gone by the select
    cell = torch.nn.LSTMCell(F + 1, 64)
    with torch.no_grad():
        cell.weight_ih.copy_(torch.cat([pol.wx, pol.wt], 1))
        cell.weight_hh.copy_(pol.wh)
        cell.bias_ih.copy_(pol.b.reshape(-1))
        cell.bias_hh.zero_()
        mv, cm, (h, c), val = pol(obs, state, es)
        mask = (es > 0).unsqueeze(1)
        x = torch.cat([obs.rows, obs.timestep.float().unsqueeze(0)]).T
        h2, c2 = cell(x, (torch.where(mask, torch.zeros(()), state[0]), torch.where(mask, torch.zeros(()), state[1])))
        assert tuple(mv.shape) == (4, n) and tuple(cm.shape) == (C, n) and tuple(h.shape) == (n, 64) and tuple(val.shape) == (n,)
        assert torch.isfinite(h).all() and torch.isfinite(c).all()
        assert (h - h2).abs().max() <= 4e-6 and (c - c2).abs().max() <= 4e-6          # float32 round-off of O(1) sums
        out = pol.w2 @ h2.T + pol.b2
        assert (mv - out[:4]).abs().max() <= 1e-5 and (cm - out[4:]).abs().max() <= 1e-5
        assert (val - (pol.wv @ h2.T + pol.bv).reshape(-1)).abs().max() <= 1e-5
        # no episode_start = nobody starts; the initial state is zeros, env-major
        st0 = pol.initial_state(n)
        assert tuple(st0[0].shape) == (n, 64) and not st0[0].any() and not st0[1].any()
        a = pol(obs, st0, None)
        b = pol(obs, (torch.ones(n, 64), torch.ones(n, 64)), torch.ones(n))
        assert torch.equal(a[0], b[0]) and torch.equal(a[2][1], b[2][1])


@pytest.mark.parametrize("F,C,odt,scale", [(7, 1, "int8", 1), (29, 2, "int32", 8), (62, 16, "float32", 1)])
def test_reference_agrees_with_the_module(F, C, odt, scale):
    """step(emulate=False) is the module in float64; step(emulate=True) stays close to it at the init scale;
    the bounds are positive and finite; every mutant moves the emulated reference."""
    n = 50
    pol = rr.make_module(F, C, 5 + F, scale)
    w = rr.weights(pol)
    rows, ts = rr.make_rows(F, n, odt, 9), np.random.default_rng(4).integers(0, 334, n) / 333.0
    h, c, es = rr.make_state(n, 2)

    class Obs(dict):
        pass
    obs = Obs()
    obs.rows, obs.timestep = torch.from_numpy(rows.astype(np.float64)), torch.from_numpy(ts)
    with torch.no_grad():
        mv, cm, (hn, cn), val = pol.double()(obs, (torch.from_numpy(h.T.astype(np.float64)), torch.from_numpy(c.T.astype(np.float64))),
                                             torch.from_numpy(es))
    ex = rr.step(w, rows, ts, h, c, es, emulate=False)
    tol = lambda x: 1e-10 * (1 + np.abs(x).max())  # noqa: E731
    assert np.allclose(ex["logits"], torch.cat([mv, cm]).numpy(), rtol=0, atol=tol(ex["logits"]))
    assert np.allclose(ex["value"], val.numpy(), rtol=0, atol=tol(ex["value"]))
    assert np.allclose(ex["h"], hn.numpy().T, rtol=0, atol=1e-12) and np.allclose(ex["c"], cn.numpy().T, rtol=0, atol=1e-12)
    em = rr.step(w, rows, ts, h, c, es)
    small = np.abs(rows.astype(np.float64)).max(axis=0) <= 2          # fp16 features are exact there
    if scale == 1:
        assert np.abs(em["h"] - ex["h"])[:, small].max() < 5e-3 and np.abs(em["logits"] - ex["logits"])[:, small].max() < 1e-2
    dh, dc = rr.state_bound(em)
    lb, vb, info = rr.logits_bound(em)
    for t in (dh, dc, lb, vb):
        assert np.isfinite(t).all() and (t > 0).all()
    assert lb.shape == (4 + C, n) and vb.shape == (n,) and dh.shape == (64, n)
    assert dh[:, small].max() < 1e-3 * scale and 0 < info["flipped"].mean() < 0.5
    for name in rr.MUTANTS:
        mu = rr.step(w, rows, ts, h, c, es, mutate=name)
        assert (np.abs(mu["h"] - em["h"]) > 0).any() or (np.abs(mu["logits"] - em["logits"]) > 0).any(), name
    with pytest.raises(ValueError):
        rr.step(w, rows, ts, h, c, es, mutate="nothing")


def test_the_sampling_cases_seed_keeps_the_reference_inside_the_cap():
    """tests/test_recurrent_seat_gpu.py excludes an (env, head) draw whose margin to a cumulative boundary is
    below 1e-5 and allows 0.5 % of them: with the case's seeds the emulated reference alone excludes fewer."""
    case = rr.sampling_case()
    em = rr.step(case["w"], case["rows"], case["ts"], case["h"], case["c"], case["es"])
    _, out = pr.pcg32(case["rng"])
    u = pr.draw_u(out)
    C = case["C"]
    excluded = 0
    for lo, hi, row in ((0, 4, 0), (4, 4 + C, 1)):
        _, margin = pr.ref_sample(em["logits"][lo:hi] / pr.LN2, u[row])
        excluded += int((margin < 1e-5).sum())
    assert excluded / (2.0 * case["n"]) <= rr.SAMPLING_CAP / 2, excluded


# ---- the code object ------------------------------------------------------------------------------
def test_the_new_unit_is_neither_first_nor_last_and_uses_no_scratch(tmp_path):
    from gym_comm_amd import build
    rec = build.LIBS["policy"]
    at = rec.sources.index("oc_policy_lstm.hip")
    assert 0 < at < len(rec.sources) - 1 and rec.sources[0] == "oc_policy.hip"
    text = open(os.path.join(build.CSRC, "oc_policy_lstm.hip")).read()
    for inc in re.findall(r'#include "(oc_\w+\.h)"', text):
        assert inc in rec.local_headers, inc
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    co = str(tmp_path / "lstm.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, "oc_policy_lstm.hip"), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    print(list(zip(names, regs)))
    assert len(names) == 9 and all("k_policy_lstm" in n for n in names), names     # 3 row types x 3 CMAX
    assert len(sizes) == 9 and max(sizes) == 0, sizes
    assert len(regs) == 9 and max(regs) <= 512, regs
    assert max(lds) == 0, lds
