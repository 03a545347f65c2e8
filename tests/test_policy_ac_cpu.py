"""The host side of the actor-critic policy kernel (include/oc_policy.h: oc_policy_mlp_ac) without
a GPU: the library's surface and argument checks, the value-row packers index by index against the
plain ones, the float64 reference of tests/policy_ac_ref.py against the torch module, and the code
object's private segment sizes."""
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
import policy_ref as pr  # noqa: E402

FP = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
VP = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib.load(lib="policy")


def test_library_exports_the_actor_critic_entry_points_and_refuses_bad_arguments():
    from gym_comm_amd import _lib
    L = _policy_lib()
    for sym in ("oc_policy_pack_w2v", "oc_policy_pack_b2v", "oc_policy_mlp_ac"):
        assert sym in _lib.LIBS["policy"].protos and getattr(L, sym) is not None
    assert L.oc_policy_abi_version() == 1
    # every check comes before any device work: these calls run without a GPU.  The pointers are
    # never dereferenced (a refused call launches nothing), so any non-NULL value stands for a tensor.
    some = 0x1000
    full = lambda **kw: _lib.PolicyAcPlayer(_lib.PolicyPlayer(some, some, some, some, None, None, None), **kw)  # noqa: E731
    one = (_lib.PolicyAcPlayer * 1)(full())
    assert L.oc_policy_mlp_ac(one, 1, some, 29, 17, 2, 64, None) != 0
    assert b"C <= 16" in L.oc_policy_last_error()
    assert L.oc_policy_mlp_ac(None, 1, some, 29, 2, 2, 64, None) != 0
    assert L.oc_policy_mlp_ac(one, 3, some, 29, 2, 2, 64, None) != 0
    assert L.oc_policy_mlp_ac(one, 1, some, 29, 2, 3, 64, None) != 0
    lone = (_lib.PolicyAcPlayer * 1)(full(move_row=some))
    assert L.oc_policy_mlp_ac(lone, 1, some, 29, 2, 2, 64, None) != 0
    assert b"together" in L.oc_policy_last_error()
    lone = (_lib.PolicyAcPlayer * 1)(full(comm_row=some))
    assert L.oc_policy_mlp_ac(lone, 1, some, 29, 2, 2, 64, None) != 0
    bare = (_lib.PolicyAcPlayer * 1)(_lib.PolicyAcPlayer(_lib.PolicyPlayer(some, some, None, some, None, None, None)))
    assert L.oc_policy_mlp_ac(bare, 1, some, 29, 2, 2, 64, None) != 0
    assert L.oc_policy_mlp_ac(one, 1, some, 29, 2, 2, (2 ** 31) // 29 + 1, None) != 0
    assert b"2^31" in L.oc_policy_last_error()
    assert L.oc_policy_mlp_ac(one, 1, some, 29, 2, 2, 0, None) == 0          # n == 0: nothing to do
    w = np.zeros((21, 64), np.float32)
    o2, ob = np.zeros((4, 64, 8), np.uint16), np.zeros((64, 16), np.float32)
    assert L.oc_policy_pack_w2v(FP(w), FP(w[0]), 17, VP(o2)) != 0
    assert L.oc_policy_pack_w2v(FP(w), None, 2, VP(o2)) != 0
    assert L.oc_policy_pack_b2v(FP(w[:, 0]), FP(w), None, FP(w[0]), 2, FP(ob)) != 0
    assert L.oc_policy_pack_b2v(FP(w[:, 0]), FP(w), FP(w[0]), FP(w[0]), 0, FP(ob)) != 0


@pytest.mark.parametrize("F,C", [(29, 2), (35, 5), (62, 16), (7, 1)])
def test_value_row_packers_index_by_index(F, C):
    """pack_w2v / pack_b2v equal pack_w2 / pack_b2 bit for bit everywhere except row 8 of the second
    product; row 8 holds -2 log2(e) wv in fp16 at element j of lanes 8 and 40 of k-step s (hidden
    unit 16 s + 8 (j >> 2) + 4 (l >> 5) + (j & 3)); register 4 of lanes 0..31 holds the folded bv."""
    L = _policy_lib()
    rng = np.random.default_rng(100 * F + C)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    for scale in (1.0, 32.0):
        w2, b2 = f32((rng.random((4 + C, 64)) * 2 - 1) * scale / 8), f32((rng.random(4 + C) * 2 - 1) * scale)
        wv, bv = f32((rng.random(64) * 2 - 1) * scale / 8), f32((rng.random(1) * 2 - 1) * scale)
        o2, o2v = np.zeros((4, 64, 8), np.uint16), np.full((4, 64, 8), 0xFFFF, np.uint16)
        ob, obv = np.zeros((64, 16), np.float32), np.full((64, 16), np.nan, np.float32)
        assert L.oc_policy_pack_w2(FP(w2), C, VP(o2)) == 0 and L.oc_policy_pack_b2(FP(b2), FP(w2), C, FP(ob)) == 0
        assert L.oc_policy_pack_w2v(FP(w2), FP(wv), C, VP(o2v)) == 0
        assert L.oc_policy_pack_b2v(FP(b2), FP(w2), FP(bv), FP(wv), C, FP(obv)) == 0
        Wv = pr.fold_w2(wv.reshape(1, 64))[0]                     # float64 of the fp16 values
        bvp = pr.fold_b2(bv, wv.reshape(1, 64))[0]
        assert np.any(Wv != 0)
        for s in range(4):
            for l in range(64):
                for j in range(8):
                    if (l & 31) == 8:
                        hid = 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)
                        assert o2[s, l, j] == 0       # the plain packing leaves the row empty
                        assert o2v[s, l, j] == np.float16(Wv[hid]).view(np.uint16), (s, l, j)
                    else:
                        assert o2v[s, l, j] == o2[s, l, j], (s, l, j)
        for l in range(64):
            for r in range(16):
                if r == 4 and l < 32:                 # row (r & 3) + 8 (r >> 2) + 4 (l >> 5) = 8
                    assert ob[l, r] == 0
                    assert obv[l, r].view(np.uint32) == np.float32(bvp).view(np.uint32), (l, r)
                else:
                    assert obv[l, r].view(np.uint32) == ob[l, r].view(np.uint32), (l, r)


@pytest.mark.parametrize("F,C,odt,scale", [(29, 2, "int8", 1), (35, 5, "float32", 4), (46, 16, "int32", 1)])
def test_reference_agrees_with_the_torch_module_in_float64(F, C, odt, scale):
    """ref_value / ref_log_prob without emulation against MLPActorCritic.forward_ac +
    torch.log_softmax in float64, and per head sum_a exp(lp(a)) = 1 to 1e-12 (with and without the
    header's roundings)."""
    n = 50
    pol = ar.make_actor_critic(F, C, 3 + F, scale)
    w, wv, bv = ar.weights(pol)
    rows, ts = ar.make_rows(F, n, odt, 5), ar.make_timesteps(n, 333, 5)

    class Obs(dict):          # what partners.rows_and_timestep reads of an ObsView
        pass
    obs = Obs()
    obs.rows, obs.timestep = torch.from_numpy(rows.astype(np.float32)), torch.from_numpy(ts)
    with torch.no_grad():
        fa = [t.numpy() for t in pol.forward_ac(obs)]             # the module itself, float32
        pol = pol.double()
        h = torch.tanh(pol.w1 @ obs.rows.double() + pol.wt * obs.timestep.unsqueeze(0) + pol.b1)
        mv, cm, val = (t.numpy() for t in (pol.w2[:4] @ h + pol.b2[:4], pol.w2[4:] @ h + pol.b2[4:],
                                            (pol.wv @ h + pol.bv).reshape(-1)))
        lsm = [torch.log_softmax(torch.from_numpy(x), dim=0).numpy() for x in (mv, cm)]
    for got, want in zip(fa, (mv, cm, val)):          # forward_ac is that function, up to float32
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-3 * (1 + np.abs(want).max())
    assert np.allclose(ar.ref_value(w, wv, bv, rows, ts, emulate=False), val, rtol=0, atol=1e-10 * (1 + np.abs(val).max()))
    g = np.random.default_rng(1)
    acts = np.stack([g.integers(0, 4, n), g.integers(0, C, n)], axis=1)
    lp, terms = ar.ref_log_prob(w, rows, ts, acts, emulate=False)
    want = lsm[0][acts[:, 0], np.arange(n)] + lsm[1][acts[:, 1], np.arange(n)]
    assert np.allclose(lp, want, rtol=0, atol=1e-10 * (1 + np.abs(want).max()))
    for emulate in (False, True):
        sums = np.zeros((2, n))
        for a in range(max(4, C)):
            _, t = ar.ref_log_prob(w, rows, ts, np.full((n, 2), a), emulate=emulate)
            sums += np.exp(t)                 # exp(-inf) = 0 past a head's range
        assert np.abs(sums - 1).max() <= 1e-12
    bad = acts.copy()
    bad[3, 1], bad[7, 0] = C, -1
    lpb, _ = ar.ref_log_prob(w, rows, ts, bad)
    assert np.isneginf(lpb[[3, 7]]).all() and np.isfinite(np.delete(lpb, [3, 7])).all()
    assert (ar.log_prob_bound(w, rows, ts, acts) > 0).all() and (ar.value_bound(w, wv, bv, rows, ts) > 0).all()


def test_actor_critic_module_carries_the_policy_weights_of_the_same_seed():
    from gym_comm_amd.vec_env import MLPActorCritic, MLPPolicy
    a, p = MLPActorCritic(5, 3, seed=11), MLPPolicy(5, 3, seed=11)
    for name in ("w1", "b1", "wt", "w2", "b2"):
        assert torch.equal(getattr(a, name), getattr(p, name)), name
    assert tuple(a.wv.shape) == (1, 64) and tuple(a.bv.shape) == (1, 1)
    assert not torch.equal(a.wv, MLPActorCritic(5, 3, seed=12).wv)
    assert a.wv.abs().max() <= 1 / 8 and a.wv.abs().max() > 0
    # the head is drawn from the SAME generator, right behind the parent's parameters and by its
    # rule (uniform in +-1/sqrt(fan-in); a bias has fan-in 1)
    g = torch.Generator().manual_seed(11)
    for t in p.parameters():
        torch.rand(t.shape, generator=g)
    for t in (a.wv, a.bv):
        want = (torch.rand(t.shape, generator=g) * 2 - 1) / float(np.sqrt(t.shape[-1]))
        assert torch.equal(t.detach(), want)
    assert [n for n, _ in a.named_parameters()] == ["w1", "b1", "wt", "w2", "b2", "wv", "bv"]
    assert not hasattr(p, "wv") and len(list(p.parameters())) == 5


def test_no_kernel_of_the_policy_library_uses_scratch(tmp_path):
    """Private segment size 0 for every kernel of liboc_policy.so, read from the code object's notes
    as test_no_built_library_uses_scratch reads them: the tail indexes its candidates with selects."""
    from gym_comm_amd import build
    tools = "/opt/rocm/lib/llvm/bin/"
    if not all(os.path.exists(tools + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    so = build.build_lib("policy")
    fat, co = str(tmp_path / "f.bin"), str(tmp_path / "k.co")
    subprocess.run([tools + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
    subprocess.run([tools + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
    notes = subprocess.run([tools + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    names = re.findall(r"\.name:\s+(\S*k_policy_mlp_ac\S*)", notes)
    assert len(names) == 18 and len(sizes) == 36          # 3 row types x 2 mappings x 3 CMAX, both kernels
    assert max(sizes) == 0, max(sizes)
