"""The host side of the MLP policy against tests/policy_ref.py, without a GPU: the reference and
the packer (oc_policy_pack_*) agree on every fp16 / fp32 value the kernel multiplies by, the
generator and its rewind (FusedMLPPartner.rewind_rng) are exact inverses over the whole uint32
range, and oc_policy_mlp refuses a batch its 32-bit element offsets cannot address."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import policy_ref  # noqa: E402


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib.load(lib="policy")


def _pcg32_scalar(s):
    """oc_policy_device.h's pcg32, one uint32 at a time in Python integers."""
    s = (s * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return s, (w >> 22) ^ w


def test_pcg32_restatement_matches_the_kernel_source_and_the_partner_constants():
    from gym_comm_amd.vec_env import FusedMLPPartner
    assert (FusedMLPPartner._PCG_MULT, FusedMLPPartner._PCG_INC) == (policy_ref.PCG_MULT, policy_ref.PCG_INC)
    src = open(os.path.join(os.path.dirname(HERE), "gym-comm_amd", "csrc", "oc_policy_device.h")).read()
    for const in (policy_ref.PCG_MULT, policy_ref.PCG_INC, policy_ref.PCG_OUT_MULT):
        assert "%du" % const in src
    states = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xDEADBEEF, 12345], np.uint64)
    s, out = policy_ref.pcg32(states)
    for k, st in enumerate(states.tolist()):
        assert (int(s[k]), int(out[k])) == _pcg32_scalar(st)
    # int32 bit patterns (the rng tensors' dtype) are the same states
    s2, out2 = policy_ref.pcg32(states.astype(np.uint32).view(np.int32))
    assert np.array_equal(s, s2) and np.array_equal(out, out2)
    u = policy_ref.draw_u(np.array([0, 255, 256, 0xFFFFFFFF], np.uint64))
    assert u.tolist() == [0.5 / 2 ** 24, 0.5 / 2 ** 24, 1.5 / 2 ** 24, 1 - 0.5 / 2 ** 24]


def test_rewind_rng_inverts_one_draw_across_the_int32_range():
    """rewind_rng works on int32 bit patterns through int64 arithmetic (wraparound at 2^32 and at
    the int32 sign): rewinding and then advancing with the host PCG32 gives back every state."""
    from gym_comm_amd.vec_env import FusedMLPPartner, MLPPolicy
    _policy_lib()
    fused = FusedMLPPartner(MLPPolicy(3, 2, seed=1), sample=True, seed=9, device="cpu")
    n = 12
    fused._buffers(n)
    special = [0, 1, 2 ** 31 - 1, -2 ** 31, -1, 2, -2, 2 ** 31 - 2, -2 ** 31 + 1,
               policy_ref.PCG_INC - 2 ** 32, 747796405, 123456789]
    orig = torch.tensor([special, special[::-1]], dtype=torch.int32)
    fused._rng.copy_(orig)
    fused.rewind_rng()
    back = fused._rng.numpy().copy()
    assert back.dtype == np.int32
    s, _ = policy_ref.pcg32(back)
    assert np.array_equal(s.astype(np.uint32).view(np.int32), orig.numpy())
    # and one advance followed by a rewind is the identity too
    adv, _ = policy_ref.pcg32(orig.numpy())
    fused._rng.copy_(torch.from_numpy(adv.astype(np.uint32).view(np.int32)))
    fused.rewind_rng()
    assert torch.equal(fused._rng, orig)
    # a greedy partner has no streams: nothing to rewind
    greedy = FusedMLPPartner(MLPPolicy(3, 2, seed=1), sample=False, seed=9, device="cpu")
    greedy._buffers(n)
    before = greedy._rng.clone()
    greedy.rewind_rng()
    assert torch.equal(greedy._rng, before)


def test_reference_rounds_exactly_as_the_packer_does():
    """Every fp16 weight the reference multiplies by is the fragment oc_policy_pack_w1 / _w2 put
    at that place (the layout restated in test_host_cpu's packer test), and b2' is the packer's
    fp32 value bit for bit -- at the default init, scaled x4 / x32, and with weights that round to
    fp16 subnormals or sit on fp16 rounding midpoints."""
    L = _policy_lib()
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rng = np.random.default_rng(17)
    cases = []
    for F, C, scale in ((1, 1, 1.0), (14, 3, 4.0), (30, 8, 1.0), (46, 9, 32.0), (47, 12, 4.0), (78, 16, 1.0)):
        cases.append((F, C, (rng.random((64, F)) * 2 - 1) * scale / np.sqrt(F),
                      (rng.random((64, 1)) * 2 - 1) * scale, (rng.random((64, 1)) * 2 - 1) * scale,
                      (rng.random((4 + C, 64)) * 2 - 1) * scale / 8, (rng.random((4 + C, 1)) * 2 - 1) * scale))
    # tiny weights (fp16 subnormals and zero after the fold), and exact fp16 midpoints before it
    F, C = 29, 5
    tiny = rng.choice([1e-9, 3e-6, -2e-5, 4e-5, 0.0], size=(64, F))
    mid = (np.float16(0.5) + np.float16(2 ** -12)).astype(np.float64) / (2 * 1.4426950408889634)
    cases.append((F, C, tiny, np.full((64, 1), mid), -tiny[:, :1], tiny[:4 + C, :].repeat(3, 1)[:, :64] * 10,
                  np.full((4 + C, 1), 1e-7)))
    for F, C, w1, wt, b1, w2, b2 in cases:
        w1, wt, b1, w2, b2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (w1, wt, b1, w2, b2))
        ks = L.oc_policy_ksteps(F)
        o1, o2 = np.zeros((2, ks, 64, 8), np.uint16), np.zeros((4, 64, 8), np.uint16)
        ob = np.zeros((64, 16), np.float32)
        assert L.oc_policy_pack_w1(fp(w1), fp(wt.reshape(-1)), fp(b1.reshape(-1)), F,
                                   o1.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_w2(fp(w2), C, o2.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_b2(fp(b2.reshape(-1)), fp(w2), C, fp(ob)) == 0
        A = policy_ref.fold_w1(w1, wt, b1)                  # [64][F + 2]
        W2h = policy_ref.fold_w2(w2)                        # [4 + C][64]
        b2p = policy_ref.fold_b2(b2, w2)                    # [4 + C]
        f16 = lambda v: np.float16(v).view(np.uint16)
        row_logit = {o: o for o in range(4)}
        row_logit.update({policy_ref.comm_row(c): 4 + c for c in range(C)})
        for l in range(64):
            r, h = l & 31, l >> 5
            for j in range(8):
                for m in range(2):
                    for s in range(ks):
                        k = 16 * s + 8 * h + j
                        want = A[32 * m + r, k] if k < F + 2 else 0.0
                        assert o1[m, s, l, j] == f16(want), (F, m, s, l, j)
                for s in range(4):
                    hid = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)
                    want = W2h[row_logit[r], hid] if r in row_logit else 0.0
                    assert o2[s, l, j] == f16(want), (C, s, l, j)
            for reg in range(16):
                o = (reg & 3) + 8 * (reg >> 2) + 4 * h
                want = np.float32(b2p[row_logit[o]]) if o in row_logit else np.float32(0)
                assert ob[l, reg].view(np.uint32) == want.view(np.uint32), (C, l, reg)


def test_reference_sampler_and_emulation_on_hand_made_cases():
    # inverse CDF: u * total against the cumulative sums, the margin to the nearest boundary
    x = np.log2(np.array([[1.0, 1.0], [2.0, 2.0], [1.0, 1.0]]))     # p = 1/4, 1/2, 1/4
    act, margin = policy_ref.ref_sample(x, np.array([0.2, 0.8]))
    assert act.tolist() == [0, 2] and np.allclose(margin, [0.05, 0.05])
    act, margin = policy_ref.ref_sample(x, np.array([0.25, 0.75]))   # on a boundary: the next action
    assert act.tolist() == [1, 2] and margin.tolist() == [0.0, 0.0]
    act, margin = policy_ref.ref_sample(np.zeros((1, 3)), np.array([0.1, 0.5, 0.9]))
    assert act.tolist() == [0, 0, 0] and np.isinf(margin).all()
    # a spread too large for 2^x: all the mass on the maximum
    act, _ = policy_ref.ref_sample(np.array([[0.0], [-300.0], [5.0], [-2000.0]]), np.array([0.999999]))
    assert act.tolist() == [2]
    # the emulated network is the exact one up to fp16 roundings; zero weights leave b2 alone
    rng = np.random.default_rng(3)
    F, C, n = 31, 4, 50
    w1 = (rng.random((64, F)) * 2 - 1) / np.sqrt(F)
    wt, b1 = rng.random(64) - 0.5, rng.random(64) - 0.5
    w2, b2 = (rng.random((4 + C, 64)) * 2 - 1) / 8, rng.random(4 + C) - 0.5
    rows = rng.integers(0, 3, (F, n)).astype(np.int32)
    ts = rng.integers(0, 334, n) / 333.0
    emu = policy_ref.ref_logits(w1, wt, b1, w2, b2, rows, ts, emulate=True)
    exact = policy_ref.ref_logits(w1, wt, b1, w2, b2, rows, ts, emulate=False)
    assert emu.shape == exact.shape == (4 + C, n)
    assert 0 < np.abs(emu - exact).max() < 2e-2
    bound, info = policy_ref.logit_bound(w1, wt, b1, w2, b2, rows, ts)
    assert bound.shape == emu.shape and (bound > 0).all() and bound.max() < 1e-3
    assert info["flipped"].mean() < 0.2           # only units next to a rounding midpoint are charged
    z = np.zeros_like(w2)
    zl = policy_ref.ref_logits(np.zeros_like(w1), 0 * wt, 0 * b1, z, b2, rows, ts)
    assert np.allclose(zl, np.float32(np.float32(1.4426950408889634) * b2.astype(np.float32)).reshape(-1, 1) * np.log(2),
                       rtol=0, atol=1e-7)


def test_policy_launcher_refuses_batches_past_32_bit_offsets():
    """F * n >= 2^31 is refused before anything is launched or dereferenced (the kernel
    addresses the rows with 32-bit element offsets); non-null dummy pointers throughout."""
    from gym_comm_amd import _lib
    L = _policy_lib()
    dummy = 0x1000
    pl = (_lib.PolicyPlayer * 2)(*[_lib.PolicyPlayer(dummy, dummy, dummy, dummy, dummy, dummy, dummy)
                                   for _ in range(2)])
    for F, n in ((29, -(-2 ** 31 // 29)), (1, 2 ** 31), (78, 2 ** 40), (29, 2 ** 31 // 29 + 1)):
        assert F * n >= 2 ** 31
        assert L.oc_policy_mlp(pl, 2, ctypes.c_void_p(dummy), F, 2, 1, n, None) == -1, (F, n)
        assert b"2^31" in L.oc_policy_last_error()
    assert 29 * (2 ** 31 // 29) < 2 ** 31       # the largest batch the GPU test runs is on the good side
