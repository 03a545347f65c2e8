"""No GPU: liboc_rollout.so (include/oc_rollout.h) builds, loads, exports what its header declares and
checks its arguments before any device work; its kernels keep everything in registers; the numpy
reference of the returns / advantages loop (tests/rollout_ref.py) pins itself against a closed form;
``RolloutSink(fused=False).compute_returns_and_advantage`` -- the torch restatement -- equals
that reference bit for bit on CPU tensors; and ``oc_rollout_add_plan`` -- the launch ``oc_rollout_add``
makes, which the GPU tests read to prove which path of the kernel a shape takes -- equals an
independent restatement and keeps its invariants over a sweep of n and F."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rollout_ref
from conftest import ROOT


def _lib_and_buf(**over):
    """The typed library and a buffer description whose pointers are non-NULL but never
    dereferenced (argument errors come before any device call)."""
    from gym_comm_amd import _lib, build
    build.build_lib("rollout")
    L = _lib.load(lib="rollout")
    fields = dict((name, 0x1000) for name, _ in _lib.RolloutBuf._fields_[:14])
    fields.update(n=64, T=4, F=3, obs_type=0)
    fields.update(over)
    return L, _lib.RolloutBuf(**fields)


def _calls(L, buf):
    p = 0x1000
    ref = None if buf is None else ctypes.byref(buf)
    return {"oc_rollout_add": lambda: L.oc_rollout_add(ref, p, p, p, p, p, p, p, None),
            "oc_rollout_add_plan": lambda: L.oc_rollout_add_plan(ref, (ctypes.c_int32 * 3)()),
            "oc_rollout_add_reward": lambda: L.oc_rollout_add_reward(ref, p, p, None),
            "oc_rollout_gae": lambda: L.oc_rollout_gae(ref, p, p, 0.99, 0.95, None)}


def test_rollout_library_exports_its_header():
    from gym_comm_amd import _lib, build
    lib = build.build_lib("rollout")
    assert os.path.exists(lib) and os.path.basename(lib) == "liboc_rollout.so"
    assert os.path.dirname(lib) == os.path.dirname(build.LIBS["hostio"].lib)
    hdr = open(os.path.join(ROOT, "include", "oc_rollout.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(_lib.LIBS["rollout"].protos)
    L = _lib.load(lib="rollout")
    for sym in _lib.LIBS["rollout"].protos:
        getattr(L, sym)
    version = int(re.search(r"#define OC_ROLLOUT_ABI_VERSION (\d+)", hdr).group(1))
    assert L.oc_rollout_abi_version() == _lib.LIBS["rollout"].abi_version == version == 1
    # the ctypes struct has the header's fields, in order
    body = re.search(r"typedef struct \{(.*?)\} oc_rollout_buf;", hdr, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [name for name, _ in _lib.RolloutBuf._fields_]


BAD = {"n <= 0": dict(n=0), "n < 0": dict(n=-5), "T <= 0": dict(T=0), "F <= 0": dict(F=0),
       "obs_type 3": dict(obs_type=3), "obs_type -1": dict(obs_type=-1),
       "slot of 2 GiB, float32": dict(F=29, n=1 << 27, obs_type=2),            # 29 * 2^27 * 4 bytes
       "slot of exactly 2 GiB, int8": dict(F=1, n=1 << 31, obs_type=1),
       "slot of exactly 2 GiB, int32": dict(F=4, n=1 << 27, obs_type=0)}


@pytest.mark.parametrize("entry", ["oc_rollout_add", "oc_rollout_add_reward", "oc_rollout_gae", "oc_rollout_add_plan"])
def test_entry_points_reject_bad_arguments_before_any_device_work(entry):
    L, _ = _lib_and_buf()
    rc = _calls(L, None)[entry]()                                   # a NULL buffer pointer
    assert rc != 0
    assert entry.encode() + b":" in L.oc_rollout_last_error() and b"launch" not in L.oc_rollout_last_error()
    for what, over in BAD.items():
        L, buf = _lib_and_buf(**over)
        rc = _calls(L, buf)[entry]()
        msg = L.oc_rollout_last_error()
        assert rc != 0, what
        assert msg.startswith(entry.encode() + b":"), (what, msg)
        assert b"launch" not in msg, (what, msg)                    # refused by the check, not by the runtime
    # the largest slot that is accepted is one byte short of 2 GiB: the check is on bytes
    L, buf = _lib_and_buf(F=1, n=(1 << 31) - 1, obs_type=1, ticket=0)
    assert L.oc_rollout_add(ctypes.byref(buf), 1, 1, 1, 1, 1, 1, 1, None) != 0
    assert b"ticket" in L.oc_rollout_last_error()                   # past the size check, stopped by the next one


# ---- the launch of oc_rollout_add ------------------------------------------------------------------
def _plan(L, n, F, obs_type=0):
    _, buf = _lib_and_buf(n=n, F=F, obs_type=obs_type)
    plan = (ctypes.c_int32 * 3)(-1, -1, -1)
    assert L.oc_rollout_add_plan(ctypes.byref(buf), plan) == 0, L.oc_rollout_last_error()
    return tuple(plan)


def _sweep_n():
    """A few hundred n in 1 .. 300 000: every multiple of 256 up to 4 096 and its neighbours, the
    powers of two and theirs, the sizes the env blocks first outnumber the target at (512 * 256), the
    workload's own sizes, and a geometric ladder of odd sizes between them."""
    ns = {1, 2, 63, 64, 65, 25600, 25601, 300000, 299999}
    for m in range(256, 4096 + 1, 256):
        ns |= {m - 1, m, m + 1}
    for e in range(1, 19):
        ns |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    for k in (2, 3, 100, 101, 171, 255, 256, 257, 511, 513, 1024, 1171):
        ns |= {256 * k - 1, 256 * k, 256 * k + 1}
    x = 4097.0
    while x < 300000:
        ns.add(int(x) | 1)
        x *= 1.037
    return sorted(n for n in ns if 1 <= n <= 300000)


SWEEP_F = (1, 2, 8, 9, 29, 46, 120, 500)


def test_add_plan_equals_its_restatement_and_keeps_its_invariants():
    L, _ = _lib_and_buf()
    ns = _sweep_n()
    assert 200 <= len(ns) <= 600 and all(m + d in ns for m in range(256, 4097, 256) for d in (-1, 0, 1))
    seen = set()
    for F in SWEEP_F:
        tasks = F + 7
        for n in ns:
            gx, groups, pg = plan = _plan(L, n, F)
            assert plan == rollout_ref.add_plan(n, F), (n, F)
            env_blocks = (n + 255) // 256
            assert 1 <= gx <= env_blocks, (n, F, plan)
            assert gx * groups <= 512, (n, F, plan)                        # "never more"
            assert (groups - 1) * pg < tasks <= groups * pg, (n, F, plan)  # no group empty, no task left out
            seen.add((pg == 1, pg > 8, pg > 16, groups == 1, gx < env_blocks, 2 * gx < env_blocks))
    assert len(seen) >= 8                       # the sweep is not one corner of the policy
    # the element type does not enter the launch
    assert _plan(L, 4096, 29, 1) == _plan(L, 4096, 29, 2) == _plan(L, 4096, 29, 0)


@pytest.mark.parametrize("n,F,plan,env_blocks", [
    (4096, 29, (16, 18, 2), 16),        # the group over tasks 28..29: last observation row + timestep row
    (65536, 29, (256, 2, 18), 256),     # three ADD_AHEAD blocks: 8, 8 and 2 rows
    (131072, 29, (512, 1, 36), 512),    # one workgroup column stores the whole slot
    (25600, 29, (85, 6, 6), 100),       # some workgroups stride twice, some once
])
def test_add_plan_at_the_workloads_sizes(n, F, plan, env_blocks):
    L, _ = _lib_and_buf()
    assert _plan(L, n, F) == plan == rollout_ref.add_plan(n, F)
    assert (n + 255) // 256 == env_blocks


def test_add_plan_refuses_a_null_plan_and_leaves_the_version_alone():
    L, buf = _lib_and_buf()
    assert L.oc_rollout_add_plan(ctypes.byref(buf), None) != 0
    assert L.oc_rollout_last_error() == b"oc_rollout_add_plan: NULL plan"
    assert L.oc_rollout_abi_version() == 1      # an additive name


def test_rollout_kernels_have_no_private_segment(tmp_path):
    from gym_comm_amd import build
    tools = "/opt/rocm/lib/llvm/bin/"
    if not all(os.path.exists(tools + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    so = build.build_lib("rollout")
    fat, co = str(tmp_path / "f.bin"), str(tmp_path / "k.co")
    subprocess.run([tools + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
    subprocess.run([tools + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
    notes = subprocess.run([tools + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len(sizes) == 4 and max(sizes) == 0, sizes               # add (two element sizes), add_reward, gae


def test_reference_equals_closed_form_exactly():
    r, v, es, lv, ld = rollout_ref.integer_case()
    assert v.shape == (6, 5)
    a32, r32 = rollout_ref.gae(r, v, es, lv, ld, 1.0, 1.0, np.float32)
    a64, r64 = rollout_ref.gae(r, v, es, lv, ld, 1.0, 1.0, np.float64)
    ac, rc = rollout_ref.closed_form(r, v, es, lv, ld)
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert (a32 == a64).all() and (a32 == ac).all()
    assert (r32 == r64).all() and (r32 == rc).all()
    # the case is not degenerate: episodes end inside the buffer and the bootstrap value is used
    assert ac[5, 0] == 0 + 5 - 2 and ac[5, 1] == 1 - 0 and ac[0, 4] == (3 + 0 - 1 + 2 + 0 + 1) - 4 - 1


def _fractional(T, n, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((T, n)), g.standard_normal((T, n)).astype(np.float32),
            (g.random((T, n)) < 0.3).astype(np.float32), g.standard_normal(n).astype(np.float32),
            (g.random(n) < 0.5).astype(np.float32))


def _torch_restatement_case(state, gamma, lam, explicit):
    import torch
    from gym_comm_amd.vec_env import RolloutSink
    T, n = 7, 33
    r, v, es, lv, ld = _fractional(T, n, 5)
    sink = RolloutSink(T, n, 2, device="cpu", obs_dtype=torch.float32)
    assert not sink.fused
    sink.rewards.copy_(torch.from_numpy(r))
    sink.values.copy_(torch.from_numpy(v))
    sink.episode_starts.copy_(torch.from_numpy(es))
    pos, count = {"full": (0, T), "wrapped": (3, T + 3), "partial": (T - 1, T - 1)}[state]
    sink.pos.fill_(pos)
    sink.count.fill_(count)
    kw = dict(gamma=gamma, gae_lambda=lam) if explicit else {}
    adv, ret = sink.compute_returns_and_advantage(torch.from_numpy(lv), torch.from_numpy(ld), **kw)
    assert adv.dtype == ret.dtype == torch.float32 and adv.shape == ret.shape == (T, n)
    order = rollout_ref.slots(pos, count, T)
    ea, er = rollout_ref.gae(r[order], v[order], es[order], lv, ld, gamma, lam, np.float32)
    want_a, want_r = np.zeros((T, n), np.float32), np.zeros((T, n), np.float32)     # unused slots: untouched
    want_a[order], want_r[order] = ea, er
    assert np.array_equal(adv.numpy().view(np.int32), want_a.view(np.int32))
    assert np.array_equal(ret.numpy().view(np.int32), want_r.view(np.int32))
    # float32 rounding is really in play: the float64 loop differs in the last bits somewhere
    a64, _ = rollout_ref.gae(r[order], v[order], es[order], lv, ld, gamma, lam, np.float64)
    assert (a64 != ea).any() and np.abs(a64 - ea).max() < 1e-4
    return (r[order], v[order], es[order], lv, ld), ea


@pytest.mark.parametrize("state", ["full", "wrapped", "partial"])
def test_torch_restatement_equals_the_reference_bit_for_bit_on_cpu(state):
    _torch_restatement_case(state, 0.99, 0.95, explicit=False)


def test_default_gamma_and_lambda_cannot_see_where_the_product_is_rounded():
    """Why the tests below exist: at (0.99, 0.95) the product in double, rounded, IS the float32
    product of the rounded factors."""
    assert np.float32(0.99 * 0.95) == rollout_ref.gl_float32_product(0.99, 0.95)
    for g, lam in ((0.9, 0.8), (0.995, 0.97)):
        assert np.float32(g * lam) != rollout_ref.gl_float32_product(g, lam)
    assert np.float32(np.float64(np.float32(0.9)) * 0.8) != np.float32(0.9 * 0.8)    # g rounded first, then * lambda


@pytest.mark.parametrize("gamma,lam", [(0.9, 0.8), (0.995, 0.97)])
@pytest.mark.parametrize("state", ["full", "wrapped", "partial"])
def test_torch_restatement_forms_the_product_in_double(state, gamma, lam):
    data, ea = _torch_restatement_case(state, gamma, lam, explicit=True)
    # the planted mutant -- the product formed in float32 -- is rejected on this very data
    ma, _ = rollout_ref.gae(*data, gamma, lam, np.float32, gl=rollout_ref.gl_float32_product(gamma, lam))
    assert (ma.view(np.int32) != ea.view(np.int32)).any()
