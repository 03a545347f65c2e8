"""CPU-side checks (no GPU): level compiler vs the golden static tables, the C ABI
surface, host argument handling, and the multi-process sharding/metrics path on gloo."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, compile_for, golden_files, load_golden

ALL = (golden_files("base_") + golden_files("wrap_") + golden_files("rbase_") + golden_files("rwrap_")
       + golden_files("cbase_") + golden_files("cwrap_"))


@pytest.mark.parametrize("path", ALL, ids=[os.path.basename(p) for p in ALL])
def test_level_compiler_matches_reference_static_tables(path):
    from gym_comm_amd import compiler as C, levels as L
    z, st = load_golden(path)
    place = [(x, y) for _, x, y in st["items"]] if st["level"].startswith("random-") else None
    level = L.parse_level_text(st["level"], st["level_text"]) if "level_text" in st else st["level"]
    lv = C.compile_level(level, st["num_agents"], st["max_num_timesteps"], placements=place)
    assert (lv.width, lv.height) == (st["width"], st["height"])
    assert (lv.cells == np.array(st["cells"])).all()
    assert (lv.dist == np.array(st["dist"])).all()          # World.get_path_distance_between, all pairs
    assert [list(i) for i in lv.items] == st["items"]       # world.objects iteration order
    assert [list(a) for a in lv.agents] == st["agents"]
    tid = {n: i for i, n in enumerate(L.TYPE_NAME)}
    mine = sorted((C.KIND_NAME[s.kind], s.goal_types) for s in lv.subtasks)
    ref = sorted((k, tuple(sorted(tid[n] for a in args for n in a.split("-")))) for k, args in st["subtasks"])
    assert mine == ref
    # names agree up to the order of a Merge's two arguments: where two Merge actions have the
    # same effect the reference keeps whichever its set iteration visited last (hash-seed
    # dependent, stripsworld.py:40-43), we keep a fixed one
    def norm(kind, args):
        return "%s(%s)" % (kind, ", ".join(sorted(args) if kind == "Merge" else args))
    assert sorted(norm(C.KIND_NAME[s.kind], list(s.args)) for s in lv.subtasks) == \
        sorted(norm(k, a) for k, a in st["subtasks"])
    lv2 = compile_for(st)                                    # explicit (recorded) order
    assert [[C.KIND_NAME[s.kind], list(s.args)] for s in lv2.subtasks] == st["subtasks"]
    assert [L.TYPE_NAME[t] for t in lv.pair_types[1:]] == st["recipe0_names"]
    assert lv.max_path == 2 * (lv.width + lv.height) + 1


def test_blob_layout_roundtrip():
    from gym_comm_amd import compiler as C
    lv = C.compile_level("partial-divider_tl", 3, 77, ego_allergic=True)
    b = lv.blob
    assert b[0] == C.MAGIC and b[1] == C.VERSION and b[23] == b.size
    assert list(b[2:9]) == [7, 7, 3, 4, 6, 77, 29]
    assert b[9] == 1
    lv = C.compile_level("partial-divider_tl", 3, 77, partner_allergic=True)
    assert lv.blob[9] == 0b110
    n = 49
    assert (b[b[16]:b[16] + n].reshape(7, 7) == lv.cells).all()
    assert (b[b[17]:b[17] + n * n].reshape(n, n) == lv.dist).all()


def test_level_errors():
    from gym_comm_amd import compiler as C
    with pytest.raises(FileNotFoundError):
        C.compile_level("no-such-level", 2)
    with pytest.raises(ValueError):
        C.compile_level("open-divider_tomato", 5)
    lv = C.compile_level("random-open-divider_salad_small", 2)      # nominal placement
    assert lv.random_placement and lv.scatter_items == [0, 1, 2] and len(lv.counters) == 9
    assert not C.compile_level("open-divider_tomato", 2).random_placement
    lv = C.compile_level("random-open-divider_salad_small", 2, placements=[(1, 0), (4, 1), (3, 4)])
    assert [t for t, _, _ in lv.items] == [3, 1, 0] and lv.num_subtasks == 9
    with pytest.raises(ValueError):
        C.compile_level("random-open-divider_salad_small", 2, placements=[(1, 1), (4, 1), (3, 4)])  # Floor
    with pytest.raises(ValueError):
        C.compile_level("open-divider_tomato", 2, subtask_order=[0, 0, 1])
    with pytest.raises(ValueError):
        C.compile_level("open-divider_tomato", 2, subtask_order=["Chop(Onion)", "Chop(Tomato)", "Deliver(Plate-Tomato)"])


def test_level_text_parser_matches_builtin(tmp_path):
    from gym_comm_amd import compiler as C, levels as L
    txt = "-----t-\n/     l\n/     -\n*     -\n-     -\n-     p\n-----p-\n\nSimpleTomato\n\n2 1\n4 1\n4 4\n2 4"
    (tmp_path / "mine.txt").write_text(txt)
    a = C.compile_level("mine", 2, level_dir=str(tmp_path))
    b = C.compile_level("open-divider_tomato", 2)
    assert (a.blob[2:] == b.blob[2:]).all()
    assert len(L.BUILTIN) == 19


def test_c_abi_exports_every_declared_symbol():
    """The library loads without a GPU and exports exactly what include/oc_hip.h declares."""
    from gym_comm_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "oc_hip.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(_lib.LIBS["hip"].protos)
    L = _lib.load()
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.oc_abi_version() == _lib.LIBS["hip"].abi_version == 6
    assert L.oc_timeline_begin(None, 0, 0) == -1 and b"timeline" in L.oc_last_error()    # the product build refuses
    # argument validation happens before any device work
    assert L.oc_step(None, None, None, None, None, None, 0, None, None, None, 0, None) == -1
    assert b"oc_step" in L.oc_last_error()
    bad = np.zeros(32, np.int32)
    h = ctypes.c_void_p()
    assert L.oc_level_create(bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 32, ctypes.byref(h)) == -1
    # launch policy of the fused step (host only): four waves per 64 envs up to 32768 envs, one beyond;
    # the caller's hint overrides; the value is the launch the library really takes -- the generic
    # library splits the plain variant four ways and nothing else
    if "OC_LAUNCH" not in os.environ:
        assert [L.oc_multi_step_waves(n, 0, 0) for n in (1, 4096, 32768, 32769, 131072)] == [4, 4, 4, 1, 1]
        assert [L.oc_multi_step_waves(n, 0, 1) for n in (1, 4096, 32768, 32769)] == [1, 1, 1, 1]      # generic library
        assert L.oc_multi_step_waves(4096, 2, 0) == 1            # (no two-way split in the generic library)
        assert L.oc_multi_step_waves(4096, 1, 0) == 1 and L.oc_multi_step_waves(131072, 4, 0) == 4
        assert L.oc_multi_step_waves(4096, 7, 0) == 4 and L.oc_multi_step_waves(131072, -3, 0) == 1
    # OC_LAUNCH (one knob, read at every call) forces the policy
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from gym_comm_amd import _lib; L = _lib.load(); "
            "print(L.oc_multi_step_waves(131072, 0, 0), L.oc_multi_step_waves(4096, 0, 0))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OC_LAUNCH="split=4,wt=1"),
                         capture_output=True, text=True, check=True).stdout.split()
    assert out == ["4", "4"], out
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OC_LAUNCH="wt=0"),
                         capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "1"], out                               # (the split launches store write-through)


def test_policy_library_exports_its_header_and_packs_fragments_as_documented():
    """liboc_policy.so (include/oc_policy.h) loads without a GPU and exports what its header
    declares; the host-side packers put every weight where the header says the MFMA fragments
    expect it (an index-by-index restatement of the three layouts)."""
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    hdr = open(os.path.join(ROOT, "include", "oc_policy.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_policy_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(_lib.LIBS["policy"].protos)
    L = _lib.load(lib="policy")
    for sym in declared:
        assert getattr(L, sym) is not None
    assert L.oc_policy_abi_version() == _lib.LIBS["policy"].abi_version == 1
    assert [L.oc_policy_ksteps(F) for F in (1, 14, 15, 29, 30, 31, 46, 47)] == [1, 1, 2, 2, 2, 3, 3, 4]
    rng = np.random.default_rng(5)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    f16 = lambda a: a.astype(np.float16).view(np.uint16)
    for F, C in ((29, 2), (35, 5), (62, 16), (7, 1)):
        ks = L.oc_policy_ksteps(F)
        w1 = rng.standard_normal((64, F)).astype(np.float32)
        wt, b1 = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
        w2 = rng.standard_normal((4 + C, 64)).astype(np.float32)
        b2 = rng.standard_normal(4 + C).astype(np.float32)
        o1, o2 = np.zeros((2, ks, 64, 8), np.uint16), np.zeros((4, 64, 8), np.uint16)
        ob = np.zeros((64, 16), np.float32)
        assert L.oc_policy_pack_w1(fp(w1), fp(wt), fp(b1), F, o1.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_w2(fp(w2), C, o2.ctypes.data_as(ctypes.c_void_p)) == 0
        assert L.oc_policy_pack_b2(fp(b2), fp(w2), C, fp(ob)) == 0
        # the activation's constants are folded in: 2 log2(e) into the first layer; the second takes
        # r = 1 / (2^a + 1) with -2 log2(e) W2 and starts at log2(e) (b2 + the row sum of W2)
        LE = np.float32(1.4426950408889634)
        aug = np.zeros((64, 16 * ks), np.float32)
        aug[:, :F], aug[:, F], aug[:, F + 1] = w1, wt, b1
        aug = (np.float32(2) * LE * aug).astype(np.float32)
        row_of = {o: o for o in range(4)}                       # logit -> row of the second product
        row_of.update({4 + c: 4 + (c & 3) + 8 * (c >> 2) for c in range(C)})
        w2row, b2row = np.zeros((32, 64), np.float32), np.zeros(32, np.float32)
        for logit, o in row_of.items():
            w2row[o] = (np.float32(-2) * LE * w2[logit]).astype(np.float32)
            folded = w2row[o].astype(np.float16).astype(np.float32)
            b2row[o] = LE * b2[logit] - np.float32(0.5) * np.float32(sum(float(v) for v in folded))
        for l in range(64):
            r, h = l & 31, l >> 5
            for j in range(8):
                for m in range(2):
                    for s_ in range(ks):
                        assert o1[m, s_, l, j] == f16(aug[32 * m + r, 16 * s_ + 8 * h + j])
                for s_ in range(4):
                    assert o2[s_, l, j] == f16(w2row[r, 16 * s_ + 8 * (j >> 2) + 4 * h + (j & 3)])
            for reg in range(16):
                assert abs(ob[l, reg] - b2row[(reg & 3) + 8 * (reg >> 2) + 4 * h]) < 1e-5
    assert L.oc_policy_pack_w2(fp(np.zeros((21, 64), np.float32)), 17, o2.ctypes.data_as(ctypes.c_void_p)) != 0
    assert b"C <= 16" in L.oc_policy_last_error()
    assert L.oc_policy_mlp(None, 1, None, 29, 2, 0, 0, None) != 0      # argument errors before any launch


def test_hostio_library_exports_its_header():
    """liboc_hostio.so (include/oc_hostio.h: the numpy boundary's pack kernel) loads without a
    GPU, exports what its header declares, and sizes its buffer as documented."""
    from gym_comm_amd import _lib, build
    build.build_lib("hostio")
    hdr = open(os.path.join(ROOT, "include", "oc_hostio.h")).read()
    declared = re.findall(r"OC_API\s+[\w\s\*]+?\b(oc_\w+)\s*\(", hdr)
    assert sorted(declared) == sorted(_lib.LIBS["hostio"].protos)
    L = _lib.load(lib="hostio")
    assert L.oc_hostio_abi_version() == _lib.LIBS["hostio"].abi_version == 1
    n = 1000
    assert L.oc_pack_host_bytes(8, 4, 17, 1, 1, 1, 1, n) == n * (8 * 8 + 8 + 4 * 4 + 4 + 4 + 4 + 4 + 17)
    assert L.oc_pack_host_bytes(8, 4, 17, 0, 0, 0, 0, n) == n * (8 * 8 + 4 * 4 + 4 + 17)
    assert L.oc_pack_host(None, 0, 29, None, 8, 4, 17, None, None, None, None, None, None, 0, None) != 0
    assert b"oc_pack_host" in L.oc_hostio_last_error()


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gym_comm_amd._lib import OcError
    from gym_comm_amd.batched import BatchedOvercooked
    with pytest.raises(OcError):
        BatchedOvercooked("open-divider_tomato", num_envs=4, device="cpu")
    with pytest.raises(Exception):
        BatchedOvercooked("open-divider_tomato", num_envs=4, device="cuda")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gym-comm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("# oracle", "").replace("CPU oracle", "").replace(
                    "test oracle", "").replace("the oracle", "").replace("oracle/", "").replace(
                    "oracle)", ""), (f, "product code must not reference the oracle package")


def test_unpack_state_roundtrip():
    from gym_comm_amd.state import unpack_state
    A, M, S = 2, 4, 3
    w = np.zeros((A + M + 2, 2), np.int64)
    for e in range(2):
        w[0, e] = 2 | (1 << 4)
        w[1, e] = 5 | (5 << 4) | ((0 + 1) << 8 if e == 1 else 0)
        for i in range(M):
            w[A + i, e] = (i + 1) | (i << 4) | (i << 9) | (i << 16)
    for i in (0, 2):                                      # env 1: items 0+2 merged, held by agent 1
        w[A + i, 1] = 5 | (5 << 4) | ((1 << 8) if i == 0 else 0) | (0 << 9) | (2 << 12) | (4 << 16)
    w[0, 1] |= 17 << 16
    w[1, 1] |= 1 << 16
    w[A + M, 1] = 0b101
    w[A + M + 1, 1] = 0b010
    u = unpack_state(w, A, M, S)
    assert u["order"].tolist() == [[0, 1, 2, 3], [1, 3, 0, -1]]
    assert u["nobj"].tolist() == [4, 3]
    assert u["agents"][1].tolist() == [[2, 1, -1], [5, 5, 0]]
    assert u["items"][1][2].tolist() == [5, 5, 0, 0, 1]
    assert u["t"].tolist() == [0, 17] and u["completed"][1].tolist() == [1, 0, 1]
    assert u["goal_count"][1].tolist() == [0, 1, 0] and u["merge_counter"].tolist() == [0, 1]


def test_shard_partition():
    from gym_comm_amd.dist import shard
    for total, world in ((8 * 131072, 8), (4096, 3), (5, 8), (0, 2)):
        got = [shard(total, r, world) for r in range(world)]
        assert sum(c for _, c in got) == total
        pos = 0
        for s, c in got:
            assert s == pos
            pos += c
        assert max(c for _, c in got) - min(c for _, c in got) <= 1
    with pytest.raises(ValueError):
        shard(10, 2, 2)


_WORKER = r"""
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
import gym_comm_amd
from gym_comm_amd import dist as ocdist
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
start, count = ocdist.shard(1001, rank, world)
local = torch.tensor([count * 10, rank + 1, rank, 3 * count, 7, 0, 0, 0], dtype=torch.int64)
g = ocdist.gather_rollout_metrics(local, 1.0 + rank)
assert g["elapsed_s"] == float(world), g
assert g["total"]["env_steps"] == 10010, g
assert g["total"]["episodes"] == sum(range(1, world + 1)), g
assert len(g["per_rank"]) == world and g["per_rank"][rank][1] == rank + 1
assert ocdist.rank_seed(5, rank) != ocdist.rank_seed(5, (rank + 1) %% world)
assert ocdist.reduce_max([1.0 + rank, 5.0 - rank]) == [float(world), 5.0]
dist.barrier(); dist.destroy_process_group()
open(os.path.join(%r, "rank_%%d.ok" %% rank), "w").write("ok")
"""


def test_metrics_allgather_two_ranks_gloo(tmp_path):
    """world_size 2 on gloo: the N>1 path (shard + end-of-rollout all-gather + max-time)."""
    import socket
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % (ROOT, str(tmp_path)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
         "--master-addr", "127.0.0.1", "--master-port", port, str(script)],
        env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "rank_0.ok").exists() and (tmp_path / "rank_1.ok").exists()


def _create(L, blob):
    h = ctypes.c_void_p()
    blob = np.ascontiguousarray(blob, dtype=np.int32)
    rc = L.oc_level_create(blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(blob.size), ctypes.byref(h))
    return rc, L.oc_last_error().decode()


def test_level_validation_happens_before_any_device_work():
    """oc_level_create rejects unsupported levels with OC_E_BADARG (-1) on a machine without
    a GPU; a valid level only fails later, at the device step, with OC_E_NODEVICE (-2)."""
    import torch
    from gym_comm_amd import _lib, compiler as C, levels as L
    lib = _lib.load()
    ok = C.compile_level("open-divider_tomato", 2, 100)
    rc, msg = _create(lib, ok.blob)
    assert rc == (0 if torch.cuda.is_available() else -2), msg
    # a level that repeats a food type runs in the library's "dup" mode (multiset objects, two
    # more state words): no rejection; four of one type exceed the packed item words
    two = C.compile_level(L.parse_level_text(
        "two-tomatoes", "-t---t-\n/     l\n/     -\n*     -\n-     -\n-     p\n-----p-\n\nSimpleTomato\n\n2 1\n4 1"), 2, 100)
    assert two.has_dup and two.hip_supported and not ok.has_dup
    slot, gi, dup = _lib.subtask_info(two.blob)
    assert dup and sorted(slot) == [0, 1, 2] and len(set(gi)) == 2
    assert _lib.subtask_info(ok.blob) == ([0, 1, 2], [0, 1, 1], False)      # canonical order: identity
    rev = C.compile_level("open-divider_tomato", 2, 100, subtask_order=[2, 1, 0])
    assert _lib.subtask_info(rev.blob)[0] == [2, 1, 0]
    from gym_comm_amd import specialize as _sp
    assert _sp.spec_header_text(rev.blob) == _sp.spec_header_text(ok.blob)  # one library for every order
    rc, msg = _create(lib, two.blob)
    assert rc == (0 if torch.cuda.is_available() else -2), msg
    from gym_comm_amd import specialize
    assert "OC_SPEC_HDR" in specialize.spec_header_text(two.blob)
    four = C.compile_level(L.parse_level_text(
        "four-tomatoes", "-t-t-t-\n/     t\n/     -\n*     -\n-     -\n-     p\n-----p-\n\nSimpleTomato\n\n2 1\n4 1"), 2, 100)
    assert not four.hip_supported
    rc, msg = _create(lib, four.blob)
    assert rc == -1 and "three" in msg
    bad = ok.blob.copy(); bad[4] = 1                       # one agent
    assert _create(lib, bad)[0] == -1
    bad = ok.blob.copy(); bad[23] += 1                     # wrong total length
    assert _create(lib, bad)[0] == -1
    bad = ok.blob.copy(); bad[1] = 1                       # old blob version
    assert _create(lib, bad)[0] == -1


def test_specialised_library_refuses_other_levels():
    import torch
    from gym_comm_amd import _lib, compiler as C, specialize
    a = C.compile_level("open-divider_tomato", 2, 100)
    b = C.compile_level("full-divider_salad", 2, 100)
    path = specialize.ensure(a.blob)
    if path is None:
        pytest.skip("hipcc unavailable and no cached specialisation")
    lib = _lib.load(path)
    assert lib.oc_is_specialized() == 2 and _lib.load().oc_is_specialized() == 0      # a "level" library
    rc, msg = _create(lib, b.blob)
    assert rc == -1 and "different level" in msg
    rc, msg = _create(lib, a.blob)
    assert rc == (0 if torch.cuda.is_available() else -2), msg
    # T and the ALLERGIC flags are run-time arguments: same specialisation
    c = C.compile_level("open-divider_tomato", 2, 500, ego_allergic=True)
    assert specialize.spec_key(c.blob) == specialize.spec_key(a.blob)
    # ... and so is the subtask order (the reference's changes with PYTHONHASHSEED): the library
    # keeps subtask bits in its own canonical order and permutes the observation rows
    d = C.compile_level("open-divider_tomato", 2, 100, subtask_order=[2, 0, 1])
    assert specialize.spec_key(d.blob) == specialize.spec_key(a.blob)
    rc, msg = _create(lib, d.blob)
    assert rc == (0 if torch.cuda.is_available() else -2), msg
    text = specialize.spec_header_text(a.blob)
    assert text.startswith("// generated") and "constexpr LevelHdr OC_SPEC_HDR" in text


def test_env_args_json_loader(tmp_path):
    from gym_comm_amd.arglist import load_env_args
    cfg = {"level": "random-salad-superwide", "num_agents": 2, "max_num_timesteps": 900,
           "env_config": {}, "hyperparams": {"n_steps": 5000}, "communication_on": True,
           "num_communication": 100, "ego_led": False, "fow_radius": 2, "wandb": True}
    p = tmp_path / "env_args.json"
    p.write_text(__import__("json").dumps(cfg))
    a = load_env_args(str(p))
    assert (a.level, a.num_agents, a.max_num_timesteps, a.num_communication) == (
        "random-salad-superwide", 2, 900, 100)
    assert a.ego_config == {} and a.partner_config == {} and a.max_num_subtasks == 14
    assert a.communication_on is True and a.hyperparams == {"n_steps": 5000}
    b = load_env_args(dict(cfg, ego_config={"ALLERGIC": True, "BLIND": False, "CAN_MOVE": False}))
    assert b.ego_config["ALLERGIC"] is True and b.ego_config["CAN_MOVE"] is False
    with pytest.raises(KeyError):
        load_env_args({"num_agents": 2})


def test_two_fma_timestep_quotient_equals_division_exhaustively(tmp_path):
    """timestep_of() in oc_step_device.h forms t / T (overcooked_env.py:146) as
    t * RN(1/T) + one FMA residual + one FMA correction instead of an fp64 division.
    tools/div_check.c compares it with the correctly rounded quotient, bit for bit, for
    every 0 <= t <= 65535 and 1 <= T <= 65535 (the ranges the 16-bit fields allow)."""
    exe = str(tmp_path / "div_check")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tools", "div_check.c"),
                           "-o", exe, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    assert "mismatches: 0" in out, out


def test_level_host_header_alone(tmp_path):
    """gym-comm_amd/csrc/oc_level_host.h -- the blob compiler (with its restatement of CPython's set
    order and its stable insertion sort over raw blob words), the generator of the specialised
    header and the hand-sized table image -- is plain host C++: tests/host_header_driver.cc includes
    nothing else of the stepper and is compiled by the host compiler with the address and
    undefined-behaviour sanitizers.  For the blob of every built-in level at every agent count it
    supports, the text the driver emits for both flavours of library equals what liboc_hip.so's
    oc_level_spec_source returns, and the sanitizers report nothing."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    from gym_comm_amd import build, compiler, specialize
    from gym_comm_amd import levels as L
    build.build()
    exe = str(tmp_path / "host_header_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host_header_driver.cc"),
                           "-o", exe])
    # (ASan otherwise insists on being the first library of the process, whatever the environment preloads)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    cases = 0
    for name in sorted(L.BUILTIN):
        for agents in range(2, min(4, len(L.load_level(name).agent_starts)) + 1):
            lv = compiler.compile_level(name, agents, 500)
            blob = tmp_path / ("%s_a%d.blob" % (name, agents))
            np.ascontiguousarray(lv.blob, dtype=np.int32).tofile(str(blob))
            for geometry in (True, False):
                out = subprocess.run([exe, str(blob), "1" if geometry else "0"], capture_output=True, text=True,
                                     env=env, timeout=120)
                assert out.returncode == 0 and out.stderr == "", (name, agents, geometry, out.returncode, out.stderr)
                assert out.stdout == specialize.spec_header_text(lv.blob, geometry), (name, agents, geometry)
                cases += 1
    assert cases >= 2 * 2 * len(L.BUILTIN)


def test_no_kernel_spills_to_scratch(tmp_path):
    """Register budget of the hot kernels: the per-level specialised build of the BASELINE
    level keeps every kernel's state in VGPRs -- no scratch (a conditionally written local
    array once sent the LDS variant there) and at most 128 VGPRs (the launch geometry assumes
    one or two waves per SIMD, but never a spill)."""
    import shutil
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from gym_comm_amd import build, compiler, specialize
    lv = compiler.compile_level("open-divider_tomato", 2, 500)
    hdr = tmp_path / "spec.h"
    hdr.write_text(specialize.spec_header_text(lv.blob))
    asm = tmp_path / "k.s"
    cmd = [build.hipcc_path(), "--offload-arch=" + build.ARCH]
    cmd += [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd += ["-DOC_SPECIALIZED", '-DOC_SPEC_FILE="%s"' % hdr, "-S", "--cuda-device-only", "-o", str(asm),
            os.path.join(build.CSRC, "oc_kernels.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"; ScratchSize: (\d+)", text)]
    vgprs = [int(v) for v in re.findall(r"; NumVgprs: (\d+)", text)]
    assert len(scratch) >= 10 and len(scratch) == len(vgprs)
    assert max(scratch) == 0, scratch
    assert max(vgprs) <= 128, vgprs
    # the fused step kernel's leading scalars arrive as preloaded kernel arguments
    assert re.search(r"k_multi_step.*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", text, re.S)
    pre = [int(v) for v in re.findall(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", text)]
    assert max(pre) >= 10, pre


def test_no_built_library_uses_scratch(tmp_path):
    """Every kernel of every library build() produced -- the generic one and all specialised
    level / structure libraries -- runs without a private segment (read from the code objects'
    metadata).  A split launch of the generic fused step once kept a 984-byte private copy of its
    argument block per lane (17 us per step instead of 6.8) and no test noticed."""
    import glob
    from gym_comm_amd import build, specialize
    tools = "/opt/rocm/lib/llvm/bin/"
    if not all(os.path.exists(tools + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    libs = [os.path.join(build.CSRC, "liboc_hip.so")] + sorted(glob.glob(os.path.join(specialize.SPEC_DIR, "*.so")))
    libs = [l for l in libs if os.path.exists(l)]
    if not libs:
        pytest.skip("nothing built")
    kernels = 0
    for k, so in enumerate(libs):
        fat, co = str(tmp_path / ("f%d.bin" % k)), str(tmp_path / ("k%d.co" % k))
        subprocess.run([tools + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
        subprocess.run([tools + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
        notes = subprocess.run([tools + "llvm-readelf", "--notes", co], capture_output=True, text=True,
                               check=True).stdout
        sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
        assert sizes and max(sizes) == 0, (os.path.basename(so), max(sizes))
        kernels += len(sizes)
        os.remove(fat), os.remove(co)
    assert kernels >= 20 * len(libs)


def test_no_jit_compile_under_a_profiler(monkeypatch, tmp_path):
    """Under rocprofv3 the process has already initialised the GPU and hipcc's exec chain would
    inherit the profiler's preload: specialize.ensure() must not compile there (cached
    libraries still load), and the compiler children never see the profiler's variables."""
    from gym_comm_amd import compiler as C, specialize
    # a STRUCTURE nobody pre-built (a Tomato and three Plates); a new map of a known structure
    # would simply load that structure's library
    txt = "-------\n/  t  p\n/     -\n*     -\n-     -\n-     p\n-----p-\n\nSimpleTomato\n\n2 1\n4 1"
    (tmp_path / "uncached.txt").write_text(txt)
    lv = C.compile_level("uncached", 2, level_dir=str(tmp_path))
    assert not os.path.exists(specialize.spec_lib_path(lv.blob))
    monkeypatch.setenv("ROCP_TOOL_LIBRARIES", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
    assert specialize.profiler_attached()
    assert specialize.ensure(lv.blob) is None
    assert not os.path.exists(specialize.spec_lib_path(lv.blob))
    env = specialize.clean_env()
    assert "LD_PRELOAD" not in env and not any(k.startswith("ROCP") for k in env)
    cached = C.compile_level("open-divider_tomato", 2, 500)          # built by __graft_entry__.build()
    if os.path.exists(specialize.spec_lib_path(cached.blob)):
        assert specialize.ensure(cached.blob) == specialize.spec_lib_path(cached.blob)


def test_specialised_libraries_are_keyed_by_structure_not_by_map(tmp_path):
    """A specialised library folds the STRUCTURE of a level (recipes, item multiset, agent count,
    border kind); the map's geometry is a run-time argument.  So a user-made map with the recipes
    and items of a shipped level loads that level's library -- no hipcc needed -- while another
    recipe, agent count or border kind does not."""
    import torch
    from gym_comm_amd import _lib, compiler as C, specialize
    key = lambda lv: specialize.spec_key(lv.blob, geometry=False)      # the structure library
    base = C.compile_level("open-divider_tomato", 2, 100)
    # (the "level" flavour folds the map as well: one library per map)
    assert specialize.spec_key(C.compile_level("full-divider_tomato", 2, 100).blob) != specialize.spec_key(base.blob)
    assert key(C.compile_level("full-divider_tomato", 2, 100)) == key(base)
    assert key(C.compile_level("partial-divider_tomato", 2, 50)) == key(base)
    mine = "---t---\n/     -\n-  l  p\n*     -\n-     -\n--p----\n\nSimpleTomato\n\n1 1\n5 4"   # 7 x 6, our own
    (tmp_path / "mine.txt").write_text(mine)
    lv = C.compile_level("mine", 2, 100, level_dir=str(tmp_path))
    assert [t for t, _, _ in lv.items] == [t for t, _, _ in base.items] and lv.height == 6
    assert key(lv) == key(base)
    path = specialize.ensure(base.blob, geometry=False)
    if path is not None:
        lib = _lib.load(path)
        assert lib.oc_is_specialized() == 1
        rc, msg = _create(lib, lv.blob)
        assert rc == (0 if torch.cuda.is_available() else -2), msg
        rc, msg = _create(lib, C.compile_level("open-divider_salad", 2, 100).blob)
        assert rc == -1 and "structure" in msg
    assert key(C.compile_level("open-divider_tomato", 3, 100)) != key(base)        # agent count
    assert key(C.compile_level("open-divider_salad", 2, 100)) != key(base)         # recipes
    assert key(C.compile_level("random-open-divider_tomato", 2, 100)) != key(base)  # items / open border


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("oc_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_byte_accounting():
    """roofline.frac is formed with the bytes the layout moves (never above SURVEY's
    int32-per-field figure, which stays a labelled secondary rate)."""
    b = _load_bench()
    for A, M, S, C, wrapper, survey in ((2, 4, 3, 2, True, 536), (2, 4, 9, 2, True, 680), (3, 4, 6, 2, False, 372)):
        rd, wr = b.layout_bytes_per_env_step(A, M, S, C, wrapper)
        assert b.survey_bytes_per_env_step(A, M, S, C, wrapper) == survey
        assert rd == 4 * (A + M + 2) + 4 * (4 if wrapper else A)
        assert rd + wr < survey
    # int8 observation rows: both accountings use 1-byte observation elements
    rd8, wr8 = b.layout_bytes_per_env_step(2, 4, 3, 2, True, obs_elem=1)
    assert wr8 == 296.75 - 3 * 2 * (22 + 3 + 4)
    assert b.survey_bytes_per_env_step(2, 4, 3, 2, True, obs_elem=1) == 536 - 3 * 2 * (23 + 3 + 4)


def test_bench_plain_run_times_exactly_steps_and_dumps_a_fixed_sample(tmp_path):
    """A plain run times --steps steps once and measures nothing beyond the headline (--full adds it);
    --dump-outputs writes float32 / float64 arrays, within its byte budget the same seeded sample of
    envs for every array."""
    import torch
    b = _load_bench()
    a = b.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.reps == 1 and not a.full and a.dump_outputs is None
    a = b.parse(["--steps", "20", "--full", "--dump-outputs", str(tmp_path)])
    assert a.full and a.dump_outputs == str(tmp_path)
    n = 1000
    outs = {"obs": torch.arange(2 * 3 * n, dtype=torch.int32).view(2, 3, n) % n,
            "timestep": torch.arange(n, dtype=torch.float64) / 7, "done": torch.arange(n, dtype=torch.int32) % 2,
            "rows8": (torch.arange(n) % 100).to(torch.int8)}
    assert b.dump_outputs(outs, str(tmp_path / "all")) == {"obs": [2, 3, n], "timestep": [n], "done": [n], "rows8": [n]}
    for k, v in outs.items():
        got = np.load(str(tmp_path / "all" / (k + ".npy")))
        assert got.dtype == (np.float64 if k == "timestep" else np.float32)
        assert np.array_equal(got, v.numpy())
    full_bytes = 4 * (6 * n) + 8 * n + 4 * n + 4 * n
    shapes = b.dump_outputs(outs, str(tmp_path / "s1"), limit=full_bytes // 4)
    b.dump_outputs(outs, str(tmp_path / "s2"), limit=full_bytes // 4)
    m = shapes["done"][0]
    assert 0 < m <= n // 4 and shapes["obs"] == [2, 3, m]
    got = {k: np.load(str(tmp_path / "s1" / (k + ".npy"))) for k in outs}
    assert sum(x.nbytes for x in got.values()) <= full_bytes // 4
    idx = got["obs"][0, 0].astype(np.int64)                 # obs[0][0][e] == e: the sampled env indices
    assert (np.diff(idx) > 0).all()
    assert np.array_equal(got["timestep"], outs["timestep"].numpy()[idx])
    assert np.array_equal(got["done"], outs["done"].numpy()[idx].astype(np.float32))
    for k in outs:                                          # seeded: the same sample every time
        assert np.array_equal(got[k], np.load(str(tmp_path / "s2" / (k + ".npy"))))


def test_bench_never_reports_one_gpu_for_an_n_gpu_request(monkeypatch, capsys):
    """`python bench.py --gpus N` without a launcher starts N ranks through torch.distributed.run
    and relays rank 0's line ONLY if it says n_gpus == N (VERDICT r1 / ADVICE r1)."""
    import json
    import subprocess
    from types import SimpleNamespace
    b = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, stdout=None):
        seen["cmd"], seen["env"] = cmd, env
        return SimpleNamespace(returncode=0, stdout=(json.dumps({"n_gpus": seen["report"], "value": 1.0}) + "\n").encode())

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])
    args = b.parse(["--gpus", "4", "--steps", "20", "--warmup", "5"])
    seen["report"] = 4
    assert b.spawn_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert json.loads(capsys.readouterr().out.strip())["n_gpus"] == 4
    seen["report"] = 1                               # a run that silently measured one GPU
    assert b.spawn_ranks(args) != 0
    assert capsys.readouterr().out.strip() == ""
