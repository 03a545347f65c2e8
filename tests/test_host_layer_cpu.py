"""No GPU: the host layer's pure parts.  ``hostio.pack_plan`` makes the plan the numpy boundary's pack
kernels are launched with, ``partners.pack_fragments`` is the packing both fused seats upload, and a
``PreparedStep`` destroys its native handle once."""
import ctypes

import numpy as np
import pytest
import torch

from test_hostio_mapped_gpu import _salad_widths

PARTS = ("b64", "ret", "b32", "ts", "rew", "done", "len", "b8")       # include/oc_hostio.h: the packed step's order


def _hostio():
    from gym_comm_amd import _lib, build
    build.build_lib("hostio")
    return _lib.load(lib="hostio")


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "no-stats"])
def test_pack_plan_is_the_restated_salad_plan_with_contiguous_offsets(stats):
    from gym_comm_amd.batched import obs_layout
    from gym_comm_amd.hostio import pack_plan
    F, widths, words = _salad_widths()
    assert F == 37 and widths == (8, 4, 25)
    n, s = 777, int(stats)
    layout = obs_layout(9, 3)
    p = pack_plan(layout, F, n, stats)
    assert p.width == widths and p.stats is stats
    assert p.words.dtype == np.int32 and np.array_equal(p.words, words)
    # every key's columns: its own block, as many as it has rows, in row order
    for k, (lo, hi) in layout.items():
        blk, c0, c1 = p.cols[k]
        assert c1 - c0 == hi - lo and [int(w) for w in p.words[lo:hi]] == [(blk << 16) | c for c in range(c0, c1)], k
    sizes = (n * 8 * 8, n * 8 * s, n * 4 * 4, n * 4, n * 4, n * 4, n * 4 * s, n * 25)
    assert p.off._fields == PARTS
    at = 0
    for name, size in zip(PARTS, sizes):
        assert getattr(p.off, name) == (at, at + size), name
        at += size
    assert p.total == at == _hostio().oc_pack_host_bytes(8, 4, 25, 1, s, 1, s, n)
    if stats:
        assert p.total == 100233


@pytest.mark.parametrize("S,C,n", [(9, 3, 1), (9, 0, 777), (4, 0, 1), (14, 16, 130)])
def test_pack_plan_widths_sum_to_F_for_one_env_and_without_comm(S, C, n):
    from gym_comm_amd.batched import obs_layout
    from gym_comm_amd.hostio import pack_plan
    F = 22 + S + 2 * C
    for stats in (True, False):
        p = pack_plan(obs_layout(S, C), F, n, stats)
        assert sum(p.width) == F and p.width[0] == 8 and p.width[1] == 4
        # every column of every block is named once
        assert sorted(int(w) for w in p.words) == [(b << 16) | c for b in range(3) for c in range(p.width[b])]
        assert p.off.b64[0] == 0 and p.off.b8[1] == p.total
        assert p.total == _hostio().oc_pack_host_bytes(*p.width, 1, int(stats), 1, int(stats), n)


def _direct(L, pol, value_head):
    """The packers called directly on the module's float32 weights."""
    f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    F, C = pol.w1.shape[1], pol.C
    w1, wt, b1, w2, b2 = f32(pol.w1), f32(pol.wt).ravel(), f32(pol.b1).ravel(), f32(pol.w2), f32(pol.b2).ravel()
    o1 = np.zeros((2, L.oc_policy_ksteps(F), 64, 8), np.uint16)
    o2, ob = np.zeros((4, 64, 8), np.uint16), np.zeros((64, 16), np.float32)
    assert L.oc_policy_pack_w1(fp(w1), fp(wt), fp(b1), F, o1.ctypes.data_as(ctypes.c_void_p)) == 0
    if value_head:
        wv, bv = f32(pol.wv).ravel(), f32(pol.bv).ravel()
        assert L.oc_policy_pack_w2v(fp(w2), fp(wv), C, o2.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_b2v(fp(b2), fp(w2), fp(bv), fp(wv), C, fp(ob)) == 0
    else:
        assert L.oc_policy_pack_w2(fp(w2), C, o2.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_b2(fp(b2), fp(w2), C, fp(ob)) == 0
    return o1, o2, ob


def test_pack_fragments_is_the_packers_output_and_touches_no_device(monkeypatch):
    from gym_comm_amd import _lib, build
    from gym_comm_amd.partners import MLPActorCritic, MLPPolicy, pack_fragments
    build.build_lib("policy")
    L = _lib.load(lib="policy")

    def no_cuda(*a, **k):
        raise AssertionError("a CUDA call")
    for name in ("_lazy_init", "current_device", "current_stream", "synchronize"):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    monkeypatch.setattr(_lib, "call", no_cuda)              # every launch of this package goes through it
    plain, ac = MLPPolicy(9, 3, seed=3), MLPActorCritic(9, 3, seed=3)
    got_p, got_v = pack_fragments(L, plain), pack_fragments(L, ac, value_head=True)
    for got, want in ((got_p, _direct(L, plain, False)), (got_v, _direct(L, ac, True)),
                      (pack_fragments(L, ac), _direct(L, ac, False))):
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert [a.dtype for a in got_p] == [np.uint16, np.uint16, np.float32]
    assert got_p[0].shape == (2, L.oc_policy_ksteps(37), 64, 8) and got_p[1].shape == (4, 64, 8) and got_p[2].shape == (64, 16)
    # the module's first layer is the same, so is its fragment
    assert np.array_equal(got_p[0], got_v[0])
    # the value head is row 8 of the second product (include/oc_policy.h): in o2 [4][64][8] it is lanes 8
    # and 40 of every k-step, in ob [64][16] register 4 of lanes 0..31.  Those differ, nothing else does
    value_lanes = [lane for lane in range(64) if lane & 31 == 8]
    other_lanes = [lane for lane in range(64) if lane & 31 != 8]
    assert value_lanes == [8, 40]
    assert np.array_equal(got_p[1][:, other_lanes], got_v[1][:, other_lanes])
    assert not got_p[1][:, value_lanes].any() and got_v[1][:, value_lanes].all()
    value_regs = np.zeros((64, 16), bool)
    value_regs[:32, 4] = True
    bits = lambda a: a.view(np.uint32)
    assert np.array_equal(bits(got_p[2])[~value_regs], bits(got_v[2])[~value_regs])
    assert (bits(got_p[2])[value_regs] != bits(got_v[2])[value_regs]).all()


class _CountingLib:
    def __init__(self):
        self.destroyed = []

    def oc_call_destroy(self, handle):
        self.destroyed.append(handle)


def test_prepared_step_close_destroys_its_handle_once():
    from gym_comm_amd.batched import PreparedStep
    lib, live, calls = _CountingLib(), [], []
    launch = lambda ego_pairs_ptr=None, pairs_int64=False: calls.append((ego_pairs_ptr, pairs_int64))
    a, b = PreparedStep(launch, lib, "handle-a", live), PreparedStep(launch, lib, "handle-b", live)
    assert live == [a, b] and not a.closed
    a(0x1000, True)
    a.launch(None, False)
    assert calls == [(0x1000, True), (None, False)]
    for _ in range(3):
        a.close()
    assert lib.destroyed == ["handle-a"] and live == [b] and a.closed and not b.closed
    with pytest.raises(RuntimeError):
        a(0x1000, False)
    with pytest.raises(RuntimeError):
        a.launch(0x1000, False)
    assert len(calls) == 2
    # the form without a native handle (a map set's): the same interface, nothing to destroy, not listed
    c = PreparedStep(launch, live=live)
    assert live == [b]
    c()
    c.close()
    c.close()
    assert lib.destroyed == ["handle-a"] and c.closed and calls[-1] == (None, False)
    b.close()
    assert lib.destroyed == ["handle-a", "handle-b"] and live == []
