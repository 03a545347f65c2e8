"""No GPU: the Python host boundary.  The loader's prototype maps agree with the headers they
restate, the one loader / one check serve every native library, the seeded PCG32 state helper
returns the bits the players were seeded with before it existed, and ``vec_env`` still exports
every name that moved out of it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = {"hip": "oc_hip.h", "policy": "oc_policy.h", "hostio": "oc_hostio.h", "rollout": "oc_rollout.h"}
DECL = re.compile(r"OC_API\s+([\w\s\*]+?)\b(oc_\w+)\s*\(([^)]*)\)\s*;")


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return [(" ".join(ret.split()), name, params.strip()) for ret, name, params in DECL.findall(text)]


def test_the_table_has_the_four_libraries_under_the_same_keys_as_the_build_table():
    from gym_comm_amd import _lib, build
    assert list(_lib.LIBS) == list(build.LIBS) == list(HEADER)
    assert [_lib.LIBS[k].env for k in HEADER] == ["OC_HIP_LIB", "OC_POLICY_LIB", "OC_HOSTIO_LIB", "OC_ROLLOUT_LIB"]
    assert [_lib.LIBS[k].abi_version for k in HEADER] == [6, 1, 1, 1]
    for name, rec in build.LIBS.items():
        assert rec.headers[0] == HEADER[name]


@pytest.mark.parametrize("lib", list(HEADER))
def test_prototype_map_agrees_with_the_header(lib):
    from gym_comm_amd import _lib
    rec = _lib.LIBS[lib]
    decls = _declarations(HEADER[lib])
    assert decls, "no OC_API declaration found"
    assert sorted(name for _, name, _ in decls) == sorted(rec.protos)
    assert rec.abi_fn in rec.protos and rec.last_error in rec.protos
    for ret, name, params in decls:
        restype, argtypes = rec.protos[name]
        count = 0 if params in ("", "void") else params.count(",") + 1
        if argtypes is None:
            assert count == 0, name
        else:
            assert len(argtypes) == count, name
        if ret == "int64_t":
            assert restype is ctypes.c_int64, name
        if ret in ("const char *", "const char*"):
            assert restype is ctypes.c_char_p, name


@pytest.mark.parametrize("seed,shape", [(0, (5,)), (1234, (2, 7)), (0x5EED + 1000003, (2, 3))])
def test_seed_helper_returns_the_bits_of_the_expression_it_replaced(seed, shape):
    from gym_comm_amd.batched import pcg32_seed_states
    want = torch.randint(0, 2 ** 31 - 1, shape, generator=torch.Generator().manual_seed(seed),
                         dtype=torch.int64).to(torch.int32)
    got = pcg32_seed_states(seed, shape, "cpu")
    assert got.dtype == torch.int32 and got.device.type == "cpu" and torch.equal(got, want)


def test_vec_env_still_exports_every_name_that_moved():
    from gym_comm_amd import hostio, learner, partners, rollout, vec_env
    home = {"ObsView": vec_env, "SPACE_DTYPE": vec_env, "ClosedLoop": vec_env, "OvercookedVecEnv": vec_env,
            "BatchEpisodeRecorder": vec_env, "RolloutSink": rollout, "RandomPartner": partners,
            "MLPPolicy": partners, "TorchPolicyPartner": partners, "RecurrentPolicyPartner": partners,
            "FusedMLPPartner": partners, "FusedActorCriticPartner": partners, "MLPActorCritic": partners,
            "PPOLearner": learner, "MappedBuffer": hostio}
    assert len(home) == 15
    for name, mod in home.items():
        assert getattr(vec_env, name) is getattr(mod, name), name
        if isinstance(getattr(mod, name), type):
            assert getattr(mod, name).__module__ == mod.__name__, name     # defined there, not passed through


@pytest.mark.parametrize("lib", list(HEADER))
def test_loader_caches_per_path_and_attaches_the_last_error_function(lib):
    from gym_comm_amd import _lib, build
    path = build.build_lib(lib)
    L = _lib.load(lib=lib)
    assert _lib.load(lib=lib) is L and _lib.load(path, lib=lib) is L
    assert L._oc_path == os.path.abspath(path)
    for sym, (restype, argtypes) in _lib.LIBS[lib].protos.items():
        fn = getattr(L, sym)
        assert fn.restype is restype, sym
        assert (None if fn.argtypes is None else list(fn.argtypes)) == argtypes, sym
    with pytest.raises(_lib.OcError) as e:
        _lib.check(-1, "what", L)
    assert str(e.value).startswith("what failed (-1): ")
    _lib.check(0, "what", L)


def test_loader_refuses_a_path_that_does_not_exist(tmp_path):
    from gym_comm_amd import _lib
    missing = str(tmp_path / "liboc_nowhere.so")
    for lib in HEADER:
        with pytest.raises(_lib.OcError) as e:
            _lib.load(missing, lib=lib)
        assert missing in str(e.value) and "there is no CPU fallback" in str(e.value)


def test_check_reports_the_librarys_own_last_error():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    build.build()
    P, H = _lib.load(lib="policy"), _lib.load()
    o2 = np.zeros((4, 64, 8), np.uint16)
    w2 = np.zeros((21, 64), np.float32)
    rc = P.oc_policy_pack_w2(w2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 17, o2.ctypes.data_as(ctypes.c_void_p))
    assert rc != 0
    with pytest.raises(_lib.OcError) as e:
        _lib.check(rc, "oc_policy_pack_w2", P)
    assert "C <= 16" in str(e.value) and str(e.value).startswith("oc_policy_pack_w2 failed (%d): " % rc)
    assert H.oc_step(None, None, None, None, None, None, 0, None, None, None, 0, None) == -1
    with pytest.raises(_lib.OcError) as e:
        _lib.check(-1, "oc_step", H)
    assert "oc_step" in str(e.value).split(": ", 1)[1] and "C <= 16" not in str(e.value)
