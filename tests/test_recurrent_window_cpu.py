"""No GPU: windows of a rollout (include/oc_policy.h, "windows of a rollout": oc_policy_window_snapshot /
oc_policy_window_gather; ``RolloutSink(state_window=W)``, ``RecurrentPPOLearner.update_windows`` / ``train_windows``).
The surface against the header, the two entry points' argument checks, the new translation unit's code object
and its place in the build, and the host logic on CPU tensors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNIT = "oc_policy_window.hip"


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib, _lib.load(lib="policy")


def _struct_fields(hdr, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") for n in re.findall(r"[\*\s,](\w+)\s*(?=,|$)", decl.strip())]


# ---- the surface -----------------------------------------------------------------------------------------------------
def test_exports_structs_and_prototypes_match_the_header():
    _l, L = _policy_lib()
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_policy_window_\w+)\s*\(", hdr)
    assert sorted(declared) == ["oc_policy_window_gather", "oc_policy_window_snapshot"]
    assert sorted(declared) == sorted(k for k in _l.LIBS["policy"].protos if k.startswith("oc_policy_window_"))
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.oc_policy_abi_version() == _l.LIBS["policy"].abi_version == 1
    assert "#define OC_POLICY_ABI_VERSION 1\n" in hdr

    def params(name):
        m = re.search(r"OC_API\s+int\s+%s\s*\(([^)]*)\)" % name, hdr)
        return [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params("oc_policy_window_snapshot") == ["const int64_t *pos", "int32_t T", "int32_t W", "const float *h",
                                                   "const float *c", "float *states", "int64_t n", "void *stream"]
    assert params("oc_policy_window_gather") == ["const oc_window_src *src", "const oc_window_batch *dst",
                                                 "const int32_t *seqs", "int32_t E", "void *stream"]
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    snap, gather = _l.LIBS["policy"].protos["oc_policy_window_snapshot"], _l.LIBS["policy"].protos["oc_policy_window_gather"]
    assert snap == (ctypes.c_int, [vp, i32, i32, vp, vp, vp, i64, vp])
    assert gather[0] is ctypes.c_int and len(gather[1]) == 5 and gather[1][2:] == [vp, i32, vp]
    assert gather[1][0]._type_ is _l.WindowSrc and gather[1][1]._type_ is _l.WindowBatch
    # the two structs, field for field
    assert _struct_fields(hdr, "oc_window_src") == [n for n, _ in _l.WindowSrc._fields_]
    assert _struct_fields(hdr, "oc_window_batch") == [n for n, _ in _l.WindowBatch._fields_]
    assert [t for _, t in _l.WindowSrc._fields_] == [vp] * 9 + [i64] + [i32] * 4
    assert [t for _, t in _l.WindowBatch._fields_] == [vp] * 10
    assert ctypes.sizeof(_l.WindowSrc) == 9 * 8 + 8 + 4 * 4 and ctypes.sizeof(_l.WindowBatch) == 10 * 8
    # the section sits between the seat's and the update's, and says what windows mean for the gradient
    at = hdr.index("/* ---- windows of a rollout")
    assert hdr.index("/* ---- the recurrent seat: an LSTM") < at < hdr.index("/* ---- the recurrent seat's PPO update")
    sec = " ".join(hdr[at:hdr.index("/* ---- the recurrent seat's PPO update")].split())
    for phrase in ("start state", "CONSTANT", "nothing flows across a window's first step", "T % W != 0 is refused",
                   "NOT checked on the device", "fastest-varying", "halted", "staging"):
        assert phrase in sec, phrase


def test_argument_checks_come_before_any_device_work_and_name_the_function():
    _l, L = _policy_lib()
    some = 0x1000          # never dereferenced: a refused call launches nothing
    src_names, dst_names = [n for n, _ in _l.WindowSrc._fields_], [n for n, _ in _l.WindowBatch._fields_]

    def src(**kw):
        base = {k: some for k, t in _l.WindowSrc._fields_ if t is ctypes.c_void_p}
        base.update(n=64, T=8, W=4, F=29, obs_type=0)
        base.update(kw)
        return _l.WindowSrc(*[base[k] for k in src_names])

    def dst(**kw):
        base = {k: some for k in dst_names}
        base.update(kw)
        return _l.WindowBatch(*[base[k] for k in dst_names])

    def refused(rc, name, text):
        err = L.oc_policy_last_error()
        assert rc != 0 and err.startswith(name + b": ") and text in err and b"launch" not in err, (rc, err, text)

    def gather(s, d, seqs, E, text):
        refused(L.oc_policy_window_gather(None if s is None else ctypes.byref(s), None if d is None else ctypes.byref(d),
                                          seqs, E, None), b"oc_policy_window_gather", text)

    gather(None, dst(), some, 8, b"NULL")
    gather(src(), None, some, 8, b"NULL")
    gather(src(), dst(), None, 8, b"NULL")
    for k, t in _l.WindowSrc._fields_:
        if t is ctypes.c_void_p:
            gather(src(**{k: None}), dst(), some, 8, b"NULL pointer in src")
    for k in dst_names:
        gather(src(), dst(**{k: None}), some, 8, b"NULL pointer in dst")
    gather(src(W=0), dst(), some, 8, b"W >= 1")
    gather(src(W=-2), dst(), some, 8, b"W >= 1")
    gather(src(T=8, W=3), dst(), some, 8, b"T % W == 0")
    gather(src(T=0), dst(), some, 8, b"T % W == 0")
    gather(src(), dst(), some, 0, b"E >= 1")
    gather(src(), dst(), some, -1, b"E >= 1")
    gather(src(n=0), dst(), some, 8, b"n >= 1")
    gather(src(F=0), dst(), some, 8, b"F + 2 <= 64")
    gather(src(F=63), dst(), some, 8, b"F + 2 <= 64")
    gather(src(obs_type=3), dst(), some, 8, b"obs_type")
    gather(src(obs_type=-1), dst(), some, 8, b"obs_type")
    gather(src(n=2 ** 25, T=4, W=4), dst(), some, 8, b"64 n must stay below 2^31")
    gather(src(n=2 ** 24, T=128, W=4), dst(), some, 8, b"T n must stay below 2^31")
    gather(src(n=64, T=2 ** 12, W=2 ** 12, F=62), dst(), some, 2 ** 14, b"W F E must stay below 2^31")

    def snapshot(pos, T, W, h, c, states, n, text):
        refused(L.oc_policy_window_snapshot(pos, T, W, h, c, states, n, None), b"oc_policy_window_snapshot", text)

    for i in range(4):
        ptrs = [some] * 4
        ptrs[i] = None
        snapshot(ptrs[0], 8, 4, ptrs[1], ptrs[2], ptrs[3], 64, b"NULL")
    snapshot(some, 8, 0, some, some, some, 64, b"W >= 1")
    snapshot(some, 8, 3, some, some, some, 64, b"T % W == 0")
    snapshot(some, 0, 1, some, some, some, 64, b"T % W == 0")
    snapshot(some, 8, 4, some, some, some, 0, b"n >= 1")
    snapshot(some, 8, 4, some, some, some, 2 ** 25, b"64 n must stay below 2^31")


# ---- the code object -----------------------------------------------------------------------------------------------
def test_the_new_unit_sits_between_the_seat_and_the_update_and_uses_no_scratch(tmp_path):
    from gym_comm_amd import build
    rec = build.LIBS["policy"]
    at = rec.sources.index(UNIT)
    assert rec.sources[at - 1] == "oc_policy_lstm.hip" and rec.sources[at + 1] == "oc_policy_rppo.hip"
    assert rec.sources[0] == "oc_policy.hip" and rec.sources[-3:] == ["oc_policy_rppo.hip", "oc_policy_rtrain.hip",
                                                                      "oc_policy_train.hip"]
    seen, todo = set(), [UNIT]
    while todo:                                                                # every local include, transitively
        name = todo.pop()
        for inc in re.findall(r'#include "(oc_\w+\.h)"', open(os.path.join(build.CSRC, name)).read()):
            assert inc in rec.local_headers, inc
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert "oc_policy_fail.h" in seen
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm binary tools not available")
    co = str(tmp_path / "window.co")
    flags = [f for f in rec.flags if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc_path(), "--offload-arch=" + build.ARCH, "--cuda-device-only", "--no-gpu-bundle-output", "-c"] + flags +
                   [os.path.join(build.CSRC, UNIT), "-o", co], check=True)
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    regs = [int(v) for v in re.findall(r"\.vgpr_count:\s+(\d+)", notes)]
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
    print(list(zip(names, regs, lds)))
    count = lambda part: sum(part in n for n in names)  # noqa: E731
    assert len(names) == 3 and (count("k_window_snapshot"), count("k_window_gather")) == (1, 2), names   # 4- and 1-byte rows
    assert len(sizes) == 3 and max(sizes) == 0, sizes
    assert len(regs) == 3 and max(regs) <= 64, regs                            # plain copies: full occupancy
    assert len(lds) == 3 and max(lds) == 0, lds


# ---- host logic ----------------------------------------------------------------------------------------------------
def test_the_sink_refuses_windows_it_cannot_record():
    from gym_comm_amd.vec_env import RolloutSink
    with pytest.raises(ValueError, match="fused=True"):
        RolloutSink(8, 4, 5, device="cpu", fused=False, state_window=4)
    for W in (3, 0, -4, 16):
        with pytest.raises(ValueError, match="does not divide"):               # refused before the device is looked at
            RolloutSink(8, 4, 5, device="cpu", fused=True, state_window=W)
    sink = RolloutSink(8, 4, 5, device="cpu")                                  # the default: nothing new
    assert sink.state_window is None and sink.lstm_states is None and len(sink.get_state()) == 3
    sig = inspect.signature(RolloutSink.__init__).parameters
    assert list(sig)[-1] == "state_window" and sig["state_window"].default is None


def test_sequence_ids_and_cuts():
    from gym_comm_amd import learner
    n, T, W = 6, 8, 4
    k, env = learner.sequence_ids(n, T, W)
    assert k.tolist() == [0] * 6 + [1] * 6 and env.tolist() == list(range(6)) * 2
    s = torch.arange(n * T // W)
    assert torch.equal(k * n + env, s)
    # ... and what an id names: slots k W .. k W + W - 1 of env `env`, a tile of 3 neighbouring ids inside one window
    slots = (k.unsqueeze(1) * W + torch.arange(W))
    assert slots[7].tolist() == [4, 5, 6, 7] and int(env[7]) == 1
    tiles = s.view(-1, 3)
    assert (k[tiles[:, 0]] == k[tiles[:, 2]]).all() and (env[tiles[:, 2]] - env[tiles[:, 0]] == 2).all()
    for bad in ((6, 8, 3), (6, 8, 0)):
        with pytest.raises(ValueError, match="does not divide"):
            learner.sequence_ids(*bad)
    # the cuts are env_cuts' with a window's W steps per sequence
    for count, W, per, want in ((128, 2, 48, [48, 48, 32]), (128, 2, None, [128]), (100, 1, 99, [99]), (100, 2, 99, [99, 1])):
        assert [E for _, E in learner.sequence_cuts(count, W, per)] == want
        assert [o for o, _ in learner.sequence_cuts(count, W, per)] == [i * (per or count) for i in range(len(want))]
        assert learner.sequence_cuts(count, W, per) == learner.env_cuts(count, W, per)
    with pytest.raises(ValueError):
        learner.sequence_cuts(128, 2, 0 - 1)


def _cpu_sink(T, n, F, W):
    """A sink on the CPU shaped as RolloutSink(fused=True, state_window=W) leaves it (the fused sink's kernels need
    a GPU; the host logic under test reads attributes only)."""
    from gym_comm_amd.vec_env import RolloutSink
    sink = RolloutSink(T, n, F, device="cpu")
    if W is not None:
        sink.state_window = W
        sink.lstm_states = torch.zeros((T // W, 2, 64, n))
    return sink


def test_the_learners_host_logic_without_a_gpu():
    from gym_comm_amd import learner
    R = learner.RecurrentPPOLearner
    ln = R.__new__(R)
    assert ln.sequences(_cpu_sink(8, 6, 5, 4)) == 12 and ln.sequences(_cpu_sink(8, 6, 5, 1)) == 48
    plain = _cpu_sink(8, 6, 5, None)
    ln.device = torch.device("cpu")
    for call in (lambda: ln.sequences(plain), lambda: ln.train_windows(plain), lambda: ln.train_graph_windows(plain, 1),
                 lambda: ln.train_windows(plain, shuffle="device"),
                 lambda: ln.update_windows(plain, torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="state_window"):                  # refused before anything else is looked at
            call()
    with pytest.raises(ValueError, match="shuffle"):
        ln.train_windows(None, shuffle="nonsense")
    # train / train_graph keep their signatures; the windowed forms mirror them
    assert list(inspect.signature(R.train_windows).parameters) == ["self", "sink", "n_epochs", "sequences_per_batch",
                                                                    "granule", "generator", "shuffle", "seed"]
    assert list(inspect.signature(R.train_graph_windows).parameters) == ["self", "sink", "n_epochs", "sequences_per_batch",
                                                                          "granule", "seed"]
    assert list(inspect.signature(R.train).parameters) == ["self", "sink", "n_epochs", "envs_per_batch", "granule",
                                                           "generator", "shuffle", "seed"]
    for name in ("update_windows", "grad_windows", "sequences", "minibatches_windows", "_sequence_windows"):
        assert name in vars(R), name
    # the window batch: one storage, laid out per minibatch size
    b = learner._WindowBatch(4, 5, 10, torch.int8, "cpu")
    assert [tuple(b.view(k, 7).shape) for k in ("obs", "timestep", "actions", "values", "h0", "c0")] == \
        [(4, 5, 7), (4, 7), (4, 2, 7), (4, 7), (64, 7), (64, 7)]
    assert b.view("obs", 7).data_ptr() == b.obs.data_ptr() and b.view("obs", 10).numel() == b.obs.numel()
    assert b.fits(4, 5, 10, torch.int8) and not b.fits(4, 5, 11, torch.int8) and not b.fits(2, 5, 4, torch.int8)
    assert not b.fits(4, 5, 4, torch.int32) and b.envs.tolist() == list(range(10)) and b.envs.dtype == torch.int32
    assert [t.data_ptr() for t in b.tensors()] == [getattr(b.c_struct, k) for k, _ in learner._lib.WindowBatch._fields_]


@pytest.mark.parametrize("W", [None, 2])
def test_the_seats_state_round_trip_with_and_without_windows(W):
    """``get_state`` / ``set_state`` carry ``lstm_states`` when the sink has windows, and only then (the seat's tensors
    stand on the CPU here, no launch is made)."""
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic
    n, T = 6, 4
    seat = FusedRecurrentPartner.__new__(FusedRecurrentPartner)
    seat.sink = sink = _cpu_sink(T, n, 5, W)
    seat.policy = LSTMActorCritic(3, 2)
    z = lambda *s: torch.zeros(s)  # noqa: E731
    seat._rng, seat.episode_start, seat.log_prob, seat.value = torch.zeros((2, n), dtype=torch.int32), z(n), z(n), z(n)
    seat.h, seat.c, seat.h0, seat.c0 = z(64, n) + 1, z(64, n) + 2, z(64, n) + 3, z(64, n) + 4
    seat.logits = None
    sink.pos.fill_(3), sink.count.fill_(3), sink.last.fill_(2)
    if W is not None:
        sink.lstm_states.copy_(torch.arange(sink.lstm_states.numel(), dtype=torch.float32).view_as(sink.lstm_states))
    st = seat.get_state(n)
    assert len(st) == 9 and len(st[4]) == (3 if W is None else 4)              # without windows: the tuple it was
    assert [int(t.item()) for t in st[4][:3]] == [3, 2, 3]
    sink.reset()
    seat.h.zero_(), seat.h0.zero_()
    if W is not None:
        want = sink.lstm_states.clone()
        sink.lstm_states.fill_(-1.0)
        assert st[4][3].data_ptr() != sink.lstm_states.data_ptr() and tuple(st[4][3].shape) == (T // W, 2, 64, n)
    seat.set_state(st)
    assert int(sink.pos.item()) == 3 and int(sink.count.item()) == 3 and (seat.h == 1).all() and (seat.h0 == 3).all()
    if W is not None:
        assert torch.equal(sink.lstm_states, want)
    else:
        assert sink.lstm_states is None
        sink.set_state(st[4][:3])                                               # a 3-tuple is still what it takes
    assert np.isfinite(seat.c.numpy()).all()
