"""No GPU: the float64 reference of the PPO update (tests/ppo_ref.py) against torch autograd; its
bounds against planted mutations, on the inputs the GPU tests use, so that no bound is vacuous; the
argument checks of oc_policy_ppo_plan / oc_policy_ppo_update / oc_policy_ppo_grad; the plan's arithmetic."""
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
import policy_ac_ref as ar  # noqa: E402
import ppo_ref as pp  # noqa: E402

TOUCHED = {"drop_sample": pp.NAMES, "ent_zero": ("w1", "wt", "b1", "w2", "b2"),
           "no_clip_mask": ("w1", "wt", "b1", "w2", "b2"), "vf_half": ("w1", "wt", "b1", "wv", "bv"),
           "biased_std": ("w1", "wt", "b1", "w2", "b2"), "one_minus_h": ("w1", "wt", "b1")}
_cases = {}


def _case(F, C, odt, scale, B, seed=None):
    key = (F, C, odt, scale, B, seed)
    if key not in _cases:
        buf = pp.make_buffer(F, C, odt, scale, seed=F + C if seed is None else seed)
        _cases[key] = pp.make_case(buf, pp.make_indices(B), pp.old_log_probs(buf))
    return _cases[key]


def _torch_loss(case, hp):
    """The loss of include/oc_policy.h written literally, float64 torch, on the exact module."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    w1, wt, b1, w2, b2 = (t(a) for a in case["w"])
    wv, bv = t(case["wv"]), t(case["bv"])
    x = torch.tensor(np.asarray(case["rows"]).astype(np.float64))
    ts = torch.tensor(np.asarray(case["ts"], np.float64)).reshape(1, -1)
    h = torch.tanh(w1 @ x + wt.reshape(-1, 1) * ts + b1.reshape(-1, 1))
    logits = w2 @ h + b2.reshape(-1, 1)
    v = (wv.reshape(1, -1) @ h).reshape(-1) + bv.reshape(-1)
    a = torch.tensor(np.asarray(case["actions"]).astype(np.int64))
    lp, H = 0.0, 0.0
    for col, (lo, hi) in enumerate(ar.HEADS):
        ls = torch.log_softmax(logits[lo:hi], dim=0)
        lp = lp + ls.gather(0, a[:, col].reshape(1, -1)).reshape(-1)
        H = H - (ls.exp() * ls).sum(dim=0)
    adv = torch.tensor(np.asarray(case["adv"], np.float64))
    ahat = (adv - adv.mean()) / (adv.std() + 1e-8)                    # torch.std: unbiased
    ratio = torch.exp(lp - torch.tensor(np.asarray(case["old_lp"], np.float64)))
    pol = -torch.min(ahat * ratio, ahat * torch.clamp(ratio, 1 - hp.clip, 1 + hp.clip)).mean()
    val = ((torch.tensor(np.asarray(case["ret"], np.float64)) - v) ** 2).mean()
    ent = -H.mean()
    loss = pol + hp.ent * ent + hp.vf * val
    loss.backward()
    return loss.item(), dict(zip(pp.NAMES, (p.grad.numpy() for p in (w1, wt, b1, w2, b2, wv, bv)))), (pol.item(), val.item(), ent.item())


@pytest.mark.parametrize("F,C,odt,scale,B", [(14, 3, "int8", 1, 33), (30, 16, "float32", 1, 210), (46, 1, "int32", 4, 300)])
def test_reference_gradient_equals_autograd(F, C, odt, scale, B):
    case, hp = _case(F, C, odt, scale, B), pp.test_hp()
    loss, want, (pol, val, ent) = _torch_loss(case, hp)
    got, stats, _ = pp.loss_and_grad(case, hp, emulate=False)
    for k in pp.NAMES:
        w = want[k].reshape(got[k].shape)
        assert np.abs(got[k] - w).max() <= 1e-10 * max(np.abs(w).max(), 1e-300), k
    for name, ref in (("loss", loss), ("policy_loss", pol), ("value_loss", val), ("entropy_loss", ent)):
        assert abs(stats[name] - ref) <= 1e-10 * max(abs(ref), 1e-300), name


@pytest.mark.parametrize("F,C,odt,scale,B,mg,seed", pp.GRAD_CASES)
def test_every_planted_mutation_leaves_the_gradient_bound(F, C, odt, scale, B, mg, seed):
    """On the GPU tests' inputs.  The mutated float64 gradient stands for a wrong kernel's; it is
    compared as tests/test_ppo_update_gpu.py compares the kernel's: unclipped against unclipped (the
    kernel's clipped gradient is checked against the reference times the kernel's OWN coefficient,
    ppo_ref.clipped_check, so the comparison is the same up to that common factor)."""
    case, hp = _case(F, C, odt, scale, B, seed), pp.test_hp()
    bound, _, ref, st = pp.grad_bound(case, hp, pp.ref_plan(B, mg))
    assert st["marginal"] == 0
    for k in pp.NAMES:
        assert np.isfinite(bound[k]).all(), k
    for mut in pp.MUTATIONS:
        got, _, _ = pp.loss_and_grad(case, hp, emulate=True, mutate=mut)
        for k in TOUCHED[mut]:
            excess = np.abs(got[k] - ref[k]) - bound[k]
            assert excess.max() > 0, (mut, k, float(excess.max()), float(bound[k].max()))


def _adam_state(case, hp, steps):
    """`steps` float64 Adam steps on the case's flat weights with the reference's clipped gradient."""
    grads, _, _ = pp.loss_and_grad(case, hp, emulate=True)
    clipped, norm, coef = pp.clip(grads, hp.max_norm)
    flat = lambda d: np.concatenate([np.asarray(d[k], np.float64).reshape(-1) for k in pp.NAMES])  # noqa: E731
    w = flat(dict(zip(pp.NAMES, list(case["w"]) + [case["wv"], case["bv"]])))
    m, v = np.zeros_like(w), np.zeros_like(w)
    for t in range(1, steps + 1):
        w, m, v = pp.adam(w, m, v, flat(clipped), t, hp)
    return w, m, v, flat(clipped), flat(grads), coef


@pytest.mark.parametrize("steps", [0, 2])
def test_every_planted_mutation_leaves_the_adam_bound(steps):
    F, C, odt, scale, B, _, seed = pp.GRAD_CASES[3]
    case, hp = _case(F, C, odt, scale, B, seed), pp.test_hp()
    w, m, v, g, g_raw, coef = _adam_state(case, hp, steps)
    assert coef < 0.9                                   # the clip is active on these inputs
    t = steps + 1
    want = pp.adam(w, m, v, g, t, hp)
    e_w, e_m, e_v = pp.adam_bound(w, m, v, g, t, hp)
    o = 0
    sizes = [64 * F, 64, 64, (4 + C) * 64, 4 + C, 64, 1]
    for mut in pp.ADAM_MUTATIONS:
        got = pp.adam(w, m, v, g_raw if mut == "no_clip_coef" else g, t, hp,
                      mutate=None if mut == "no_clip_coef" else mut)
        o = 0
        for k, size in zip(pp.NAMES, sizes):
            sl = slice(o, o + size)
            assert (np.abs(got[0][sl] - want[0][sl]) - e_w[sl]).max() > 0, (mut, k)
            o += size


def _lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib, _lib.load(lib="policy")


def test_argument_checks_come_before_any_device_work():
    _l, L = _lib()
    for sym in ("oc_policy_ppo_plan", "oc_policy_ppo_update", "oc_policy_ppo_grad"):
        assert sym in _l.LIBS["policy"].protos
    plan = (ctypes.c_int32 * 4)()
    assert L.oc_policy_ppo_plan(30, 3, 210, 0, plan) == 0
    P = 64 * 30 + 128 + 7 * 64 + 7 + 65
    assert list(plan) == [2, 1, P, 2 * (P + 8)]
    for bad in ((47, 3, 210, 0), (0, 3, 210, 0), (30, 0, 210, 0), (30, 17, 210, 0), (30, 3, 1, 0), (30, 3, 210, -1)):
        assert L.oc_policy_ppo_plan(*bad, plan) != 0, bad
        assert b"oc_policy_ppo_plan" in L.oc_policy_last_error()
    assert L.oc_policy_ppo_plan(30, 3, 210, 0, None) != 0
    some = 0x1000                                     # never dereferenced: a refused call launches nothing

    def cfg(**kw):
        c = _l.PpoCfg()
        for name, typ in _l.PpoCfg._fields_:
            if typ is ctypes.c_void_p:
                setattr(c, name, some)
        c.n, c.T, c.F, c.C, c.obs_type, c.max_groups = 70, 3, 30, 3, 2, 0
        for k, val in kw.items():
            setattr(c, k, val)
        return c
    idx = some
    for name in ("oc_policy_ppo_update", "oc_policy_ppo_grad"):
        fn = getattr(L, name)
        assert fn(None, idx, 210, None) != 0
        assert fn(ctypes.byref(cfg()), None, 210, None) != 0
        for kw, B, text in ((dict(F=47), 210, b"F + 2 <= 48"), (dict(C=17), 210, b"C <= 16"), (dict(), 1, b"B >= 2"),
                            (dict(obs_type=3), 210, b"obs_type"), (dict(T=2 ** 16, n=2 ** 15), 210, b"2^31"),
                            (dict(obs=None), 210, b"NULL"), (dict(stats=None), 210, b"NULL"),
                            (dict(w2t=None), 210, b"NULL"), (dict(hyper=None), 210, b"NULL")):
            assert fn(ctypes.byref(cfg(**kw)), idx, B, None) != 0, kw
            err = L.oc_policy_last_error()
            assert name.encode() in err and text in err, (kw, err)
    for kw in (dict(m=None), dict(step=None), dict(p_wv=None)):        # the update's own pointers
        assert L.oc_policy_ppo_update(ctypes.byref(cfg(**kw)), idx, 210, None) != 0
        assert b"master weights" in L.oc_policy_last_error()


def test_plan_covers_every_tile_and_leaves_no_group_empty():
    _l, L = _lib()
    plan = (ctypes.c_int32 * 4)()
    rng = np.random.default_rng(5)
    pairs = [(2, 0), (32, 1), (33, 1), (210, 1), (300, 3), (16384, 0), (524288, 0), (2 ** 31 - 1, 0)]
    pairs += [(int(b), int(g)) for b, g in zip(rng.integers(2, 70000, 300), rng.integers(0, 9, 300))]
    for B, mg in pairs:
        assert L.oc_policy_ppo_plan(30, 3, B, mg, plan) == 0
        G, tpw, P, scratch = list(plan)
        tiles = (B + 31) // 32
        assert (G, tpw) == pp.ref_plan(B, mg)
        assert 1 <= G <= (mg if mg else 64) and tpw >= 1
        assert 4 * G * tpw >= tiles and tiles * 32 >= B           # no tile left out
        assert 4 * (G - 1) < tiles                                # wave 0 of the last group has a tile: none empty
        assert 4 * G * (tpw - 1) < tiles                          # the last round of tiles is not all idle
        assert scratch == G * (P + 8)


def test_no_kernel_of_the_update_uses_scratch(tmp_path):
    """The update is a translation unit, and so a code object, of its own inside liboc_policy.so; its
    device code compiled alone with the library's flags: six kernels (three row types of the gradient
    kernel, the statistics, the finish with and without Adam), private segment size 0 each, and the
    gradient kernel within the 512 registers one wave per SIMD has."""
    from gym_comm_amd import build
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    rec = build.LIBS["policy"]
    assert "oc_policy_ppo.hip" in rec.sources and "oc_policy_ppo_device.h" in rec.local_headers
    co = str(tmp_path / "ppo.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, "oc_policy_ppo.hip"), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S*k_ppo_\S*)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(names) == 6 and len(sizes) == 6, names
    assert max(sizes) == 0, sizes
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    assert len(regs) == 6 and max(regs) <= 512, regs
