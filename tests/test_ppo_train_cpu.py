"""No GPU: the train sequence of include/oc_policy.h (its last section).  The epoch permutation -- the
host function against a numpy restatement of the header's prose, the header alone under the
sanitizers, its quality against numpy's shuffle; the float64 reference of the value-clipped loss
against torch autograd, and its bounds against planted mutations on the GPU tests' inputs; the entry
points' argument checks; the new translation unit's code object."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ppo_ref as pp  # noqa: E402
import ppo_train_ref as tr  # noqa: E402

SIZES = (1, 2, 3, 5, 64, 210, 4097, 65537, 2 ** 20 + 1)
SEEDS = (0, 1, 0x5EED, 0xFFFFFFFF)


def _lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib, _lib.load(lib="policy")


def _perm_host(L, seed, epoch, N):
    out = np.full(N, -7, np.int32)
    assert L.oc_policy_ppo_perm_host(seed, epoch, N, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    return out


# ---- the permutation ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_host_permutation_is_the_headers_prose_bit_for_bit(N):
    _, L = _lib()
    longest, seen = 0, []
    for seed in SEEDS:
        for epoch in range(4):
            got = _perm_host(L, seed, epoch, N)
            want, walk = tr.perm(seed, epoch, N)
            longest = max(longest, walk)
            assert np.array_equal(got, want), (seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(N, dtype=np.int32)), (seed, epoch)    # a permutation
            seen.append(got)
    print("N %d: longest walk %d passes (cap %d)" % (N, longest, tr.WALK_CAP))
    assert longest < 200
    if N >= 64:           # epochs and seeds differ (N! arrangements: no two of the 16 may coincide)
        for i in range(len(seen)):
            for j in range(i):
                assert not np.array_equal(seen[i], seen[j]), (i, j)


def test_shuffle_header_alone_is_a_bijection_under_the_sanitizers(tmp_path):
    """tests/policy_shuffle_driver.cc includes nothing but oc_policy_shuffle.h and is compiled by the
    host compiler with the address and undefined-behaviour sanitizers: a bijection for every N <= 2048
    and for the sizes above, four seeds, and no walk at the cap."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "policy_shuffle_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "policy_shuffle_driver.cc"),
                           "-o", exe])
    # (ASan otherwise insists on being the first library of the process, whatever the environment preloads)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(out.stdout[-500:])
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip().endswith("failures: 0"), out.stdout[-2000:]


def test_shuffle_quality_against_numpys():
    """N = 4096, 64 epochs: max_i |mean position of element i - (N - 1) / 2| for the Feistel shuffle
    (seed 0) and for numpy.random.Generator.permutation over 20 seeds.  The Feistel value may not
    exceed 1.5 x numpy's largest (the 1.5: slack for a statistic whose spread nobody has measured)."""
    _, L = _lib()
    N, E = 4096, 64

    def stat(perms):
        pos = np.zeros(N)
        for p in perms:
            where = np.empty(N)
            where[p] = np.arange(N)          # position of element p[k] is k
            pos += where
        return np.abs(pos / E - (N - 1) / 2.0).max()

    feistel = [stat([_perm_host(L, seed, e, N) for e in range(E)]) for seed in (0, 1, 2)]
    ref = []
    for s in range(20):
        g = np.random.default_rng(s)
        ref.append(stat([g.permutation(N) for _ in range(E)]))
    print("Feistel (seeds 0, 1, 2): %s; numpy over 20 seeds: min %.1f mean %.1f max %.1f"
          % (", ".join("%.1f" % v for v in feistel), min(ref), np.mean(ref), max(ref)))
    assert max(feistel) <= 1.5 * max(ref)


# ---- the value-clipped loss -----------------------------------------------------------------------
def _torch_value_loss(case, old_v, c):
    """value_loss of the header written literally, float64 torch, on the exact module."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    w1, wt, b1, w2, b2 = (t(a) for a in case["w"])
    wv, bv = t(case["wv"]), t(case["bv"])
    x = torch.tensor(np.asarray(case["rows"]).astype(np.float64))
    ts = torch.tensor(np.asarray(case["ts"], np.float64)).reshape(1, -1)
    h = torch.tanh(w1 @ x + wt.reshape(-1, 1) * ts + b1.reshape(-1, 1))
    v = (wv.reshape(1, -1) @ h).reshape(-1) + bv.reshape(-1)
    old = torch.tensor(np.asarray(old_v, np.float64))
    vp = old + torch.clamp(v - old, -c, c)
    val = ((torch.tensor(np.asarray(case["ret"], np.float64)) - vp) ** 2).mean()
    val.backward()
    return val.item(), dict(w1=w1.grad, wt=wt.grad, b1=b1.grad, wv=wv.grad, bv=bv.grad)


def test_value_clipped_reference_equals_autograd():
    """The value term alone (vf_coef 1, the policy and entropy terms taken out by linearity: the
    reference's gradient minus its gradient with the gate shut everywhere) against torch autograd."""
    inp = tr.vclip_inputs()
    case, old_v, c = inp["case"], inp["old_v"], inp["c"]
    hp = pp.HP(vf_coef=1.0, ent_coef=0.0)
    got, stats, info = tr.vclip_reference(case, old_v, c, hp, emulate=False)
    shut, _, _ = tr.vclip_reference(case, old_v, 1e-30, hp, emulate=False)        # every gate shut: no value gradient
    assert 40 < info["gate"].sum() < 170
    val, want = _torch_value_loss(case, old_v, c)
    assert abs(stats["value_loss"] - val) <= 1e-10 * abs(val)
    for k, w in want.items():
        g = (got[k] - shut[k]).reshape(-1)
        w = w.numpy().reshape(-1)
        assert np.abs(g - w).max() <= 1e-10 * np.abs(w).max(), k
        assert np.abs(w).max() > 0


def test_every_planted_value_clipping_mutation_leaves_the_bound():
    """On the GPU test's inputs: the reference alone keeps every sample's | |v - old_v| - c | above the
    value's error bound (so the kernel's gates are the reference's), and each mutant's gradient leaves
    the bound in every tensor the value head reaches; the two that change the loss leave value_loss's."""
    inp = tr.vclip_inputs()
    hp = pp.test_hp()
    ref, stats, info = tr.vclip_reference(inp["case"], inp["old_v"], inp["c"], hp, inp["plan"])
    print("clip_range_vf %.6f: %d of %d gates open, margin %.3e, marginal ratio samples %d"
          % (inp["c"], info["gate"].sum(), info["gate"].size, info["margin"], info["marginal"]))
    assert info["margin"] > 0 and info["marginal"] == 0
    assert 40 < info["gate"].sum() < 170
    for mut in tr.VCLIP_MUTATIONS:
        got, mstats, _ = tr.vclip_reference(inp["case"], inp["old_v"], inp["c"], hp, mutate=mut)
        for k in ("w1", "wt", "b1", "wv", "bv"):
            excess = np.abs(got[k] - ref[k]) - info["bound"][k]
            assert excess.max() > 0, (mut, k, float(excess.max()))
        if mut in ("ignored", "clamp_around_zero"):
            assert abs(mstats["value_loss"] - stats["value_loss"]) > info["stat_bound"]["value_loss"], mut


# ---- the entry points' argument checks ------------------------------------------------------------
def test_argument_checks_come_before_any_device_work():
    """NULL pointers, a granule that does not divide count, B < 2: refused with an error text that names
    the function.  The non-NULL pointers are not readable memory (and no device exists here): a call
    that got past its checks would fault."""
    _l, L = _lib()
    some = 0x1000
    for sym in ("oc_policy_ppo_perm_host", "oc_policy_ppo_train_begin", "oc_policy_ppo_epoch_begin", "oc_policy_ppo_train_step"):
        assert sym in _l.LIBS["policy"].protos

    def train(**kw):
        t = _l.PpoTrain(some, some, some, some)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def cfg(**kw):
        c = _l.PpoCfg()
        for name, typ in _l.PpoCfg._fields_:
            if typ is ctypes.c_void_p:
                setattr(c, name, some)
        c.n, c.T, c.F, c.C, c.obs_type, c.max_groups = 70, 3, 30, 3, 2, 0
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def refused(rc, name, text):
        err = L.oc_policy_last_error()
        assert rc != 0 and name in err and text in err, (rc, err)

    i32p = ctypes.POINTER(ctypes.c_int32)
    refused(L.oc_policy_ppo_perm_host(0, 0, 5, None), b"oc_policy_ppo_perm_host", b"out")
    refused(L.oc_policy_ppo_perm_host(0, 0, 0, ctypes.cast(some, i32p)), b"oc_policy_ppo_perm_host", b"N")
    refused(L.oc_policy_ppo_perm_host(0, 0, 2 ** 30 + 1, ctypes.cast(some, i32p)), b"oc_policy_ppo_perm_host", b"2^30")
    refused(L.oc_policy_ppo_perm_host(0, -1, 5, ctypes.cast(some, i32p)), b"oc_policy_ppo_perm_host", b"epoch")
    name = b"oc_policy_ppo_train_begin"
    refused(L.oc_policy_ppo_train_begin(None, None), name, b"train")
    for field in ("values", "hyper_ext", "ctl", "acc"):
        refused(L.oc_policy_ppo_train_begin(ctypes.byref(train(**{field: None})), None), name, b"NULL")
    name = b"oc_policy_ppo_epoch_begin"
    ok = ctypes.byref(train())
    refused(L.oc_policy_ppo_epoch_begin(None, some, 210, 10, 0, None), name, b"train")
    refused(L.oc_policy_ppo_epoch_begin(ctypes.byref(train(ctl=None)), some, 210, 10, 0, None), name, b"NULL")
    refused(L.oc_policy_ppo_epoch_begin(ok, None, 210, 10, 0, None), name, b"idx")
    for count, granule in ((210, 4), (210, 0), (210, -2), (0, 1), (-5, 5), (210, 211)):
        refused(L.oc_policy_ppo_epoch_begin(ok, some, count, granule, 0, None), name, b"granule")
    name = b"oc_policy_ppo_train_step"
    refused(L.oc_policy_ppo_train_step(None, ok, some, 210, None), name, b"cfg")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg()), None, some, 210, None), name, b"train")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg()), ok, None, 210, None), name, b"idx")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg()), ok, some, 1, None), name, b"B >= 2")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg(m=None)), ok, some, 210, None), name, b"master weights")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg(stats=None)), ok, some, 210, None), name, b"NULL")
    refused(L.oc_policy_ppo_train_step(ctypes.byref(cfg()), ctypes.byref(train(acc=None)), some, 210, None), name, b"NULL")
    assert ctypes.sizeof(_l.PpoTrain) == 32
    assert _l.PPO_CTL == dict(stop=0, epoch=1, updates=2, epochs=3, error=4, words=8)
    assert _l.PPO_ACC == dict(epoch_kl=0, epoch_count=1, sums=2, words=8)
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    for k, v in _l.PPO_CTL.items():
        assert re.search(r"#define OC_PPO_CTL_%s %d\b" % (k.upper(), v), hdr), k
    for k, v in _l.PPO_ACC.items():
        assert re.search(r"#define OC_PPO_ACC_%s %d\b" % (k.upper(), v), hdr), k


def test_minibatch_cuts_follow_the_existing_rule():
    total = 210
    for bs, want in ((64, [64, 64, 64, 18]), (None, [210]), (209, [209]), (105, [105, 105]), (104, [104, 104, 2])):
        assert [b for _, b in tr.cuts(total, bs)] == want
        full = torch.arange(total).split(int(bs or total))
        assert [b.numel() for b in full if b.numel() >= 2] == want


# ---- the code object ------------------------------------------------------------------------------
def test_no_kernel_of_the_train_unit_uses_scratch(tmp_path):
    """oc_policy_train.hip compiled alone with the library's flags: the three small kernels and the TRAIN
    variants of the update's five (three row types of the gradient kernel, the statistics, the finish
    with Adam); private segment size 0 each, and the gradient kernels within 512 registers.  The unit is
    the LAST of the library's sources, and the update's unit still holds its six kernels only."""
    from gym_comm_amd import build
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    rec = build.LIBS["policy"]
    assert rec.sources[-1] == "oc_policy_train.hip" and "oc_policy_shuffle.h" in rec.local_headers
    co = str(tmp_path / "train.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, "oc_policy_train.hip"), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S*k_ppo_\S*)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    print(list(zip(names, regs)))
    assert len(names) == 8 and len(sizes) == 8 and len(regs) == 8, names
    assert sum("k_ppo_grad" in n for n in names) == 3 and sum("k_ppo_finish" in n for n in names) == 1
    assert sum("k_ppo_adv" in n for n in names) == 1
    for small in ("k_ppo_train_begin", "k_ppo_epoch_close", "k_ppo_perm"):
        assert sum(small in n for n in names) == 1, small
    assert max(sizes) == 0, sizes
    assert max(regs) <= 512, regs
