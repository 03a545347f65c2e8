"""The one statement of the policy's fragment layout (gym-comm_amd/csrc/oc_policy_layout.h) without a
GPU: the header alone under a host compiler and its sanitizers, and the host packer of the learner's
transposed image against an independent index loop."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731


def test_layout_header_alone_is_a_set_of_bijections(tmp_path):
    """tests/policy_layout_driver.cc includes nothing but oc_policy_layout.h and is compiled by the host
    compiler with the address and undefined-behaviour sanitizers.  For C = 1..16 and F in {1, 14, 15, 30,
    46, 62} it checks exhaustively: logit_of_row maps exactly 4 + C rows one-to-one onto 0..3 + C and
    never row 8; the accumulator row is a bijection from (q, h) to 0..31; every (hidden, k < F + 2) is the
    source of exactly one w1 element and every other w1 element has none; every (live row, hidden) is the
    source of exactly one w2 and one w2t element; every live row feeds exactly 32 b2 elements;
    PpoLayout's seven ranges partition [0, P)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "policy_layout_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "policy_layout_driver.cc"),
                           "-o", exe])
    # (ASan otherwise insists on being the first library of the process, whatever the environment preloads)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.strip() == "failures: 0", out.stdout[-2000:]


def _policy_lib():
    from gym_comm_amd import _lib, build
    build.build_lib("policy")
    return _lib.load(lib="policy")


def w2t_by_index_loop(w2, wv, C):
    """The learner's image, float32 [2][16][64], restated index by index (the loop PPOLearner carried
    before the library packed it): element (m, t, lane) = the fp16 value of -2 log2(e) times row
    (t & 3) + 8 (t >> 2) + 4 (lane >> 5), hidden unit 32 m + (lane & 31) of [w2; wv], or 0."""
    src = np.full((2, 16, 64), -1, np.int64)
    for m in range(2):
        for t in range(16):
            for lane in range(64):
                row, hid = (t & 3) + 8 * (t >> 2) + 4 * (lane >> 5), 32 * m + (lane & 31)
                if row < 4:
                    src[m, t, lane] = row * 64 + hid
                elif row == 8:
                    src[m, t, lane] = (4 + C) * 64 + hid
                elif ((row - 4) & 7) < 4:
                    c = ((row - 4) & 3) + 4 * ((row - 4) >> 3)
                    if c < C:
                        src[m, t, lane] = (4 + c) * 64 + hid
    scale = np.float32(-2) * np.float32(1.4426950408889634)
    rows = np.concatenate([w2.reshape(-1), wv.reshape(-1)]).astype(np.float32)
    folded = (rows * scale).astype(np.float32).astype(np.float16).astype(np.float32)
    return np.where(src >= 0, folded[np.clip(src, 0, None)], np.float32(0))


@pytest.mark.parametrize("scale", [1, 32])
@pytest.mark.parametrize("F,C", [(29, 2), (35, 5), (46, 16), (7, 1)])
def test_pack_w2t_matches_the_index_loop_bit_for_bit(F, C, scale):
    L = _policy_lib()
    rng = np.random.default_rng(1000 * F + C)
    w2 = (scale * rng.standard_normal((4 + C, 64))).astype(np.float32)
    wv = (scale * rng.standard_normal(64)).astype(np.float32)
    out = np.full((2, 16, 64), np.nan, np.float32)
    assert L.oc_policy_pack_w2t(FP(w2), FP(wv), C, FP(out)) == 0
    want = w2t_by_index_loop(w2, wv, C)
    assert np.array_equal(out.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.count_nonzero(out) > 64 * (4 + C)          # (the comparison is not of zeros)


def test_pack_w2t_refuses_bad_arguments_before_touching_memory():
    """C = 0, C = 17 and a NULL w2, wv or out: refused with an error text that names the function.  The
    non-NULL pointers are not readable memory, so a packer that looked would fault."""
    L = _policy_lib()
    some = ctypes.cast(0x1000, ctypes.POINTER(ctypes.c_float))
    for w2, wv, C, out in ((some, some, 0, some), (some, some, 17, some), (None, some, 2, some),
                           (some, None, 2, some), (some, some, 2, None)):
        assert L.oc_policy_pack_w2t(w2, wv, C, out) != 0
        assert b"oc_policy_pack_w2t" in L.oc_policy_last_error()
