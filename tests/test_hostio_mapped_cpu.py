"""No GPU: the host-mapped I/O names of liboc_hostio.so (include/oc_hostio.h: oc_hostio_alloc /
oc_hostio_free, oc_pack_host_tile, oc_pack_host_tiled) check their arguments before any device work
and say who refused; without a device a valid allocation fails with the runtime's text instead of
crashing; no kernel of the library uses scratch; and ``OvercookedVecEnv(host_io=...)`` refuses an
unknown mode before the batch is constructed."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

TOOLS = "/opt/rocm/lib/llvm/bin/"
P = 0x1000      # a non-NULL pointer that is never dereferenced: argument errors come first


def _lib_hostio():
    from gym_comm_amd import _lib, build
    build.build_lib("hostio")
    return _lib.load(lib="hostio")


def _pack_args(**over):
    a = dict(obs_rows=P, obs_type=0, F=29, plan=P, w64=8, w32=4, w8=17, timestep=P, reward=P, ep_return=P,
             done=P, ep_length=P, out=P, n=64, stream=None)
    a.update(over)
    return list(a.values())


# everything oc_pack_host refuses
BAD_PACK = [dict(obs_rows=None), dict(plan=None), dict(timestep=None), dict(out=None), dict(F=0), dict(F=-3),
            dict(w64=-1), dict(w32=-1), dict(w8=-1), dict(n=-1), dict(obs_type=-1), dict(obs_type=3)]


@pytest.mark.parametrize("over", BAD_PACK, ids=lambda o: "%s=%s" % next(iter(o.items())))
def test_tiled_pack_refuses_what_the_plain_pack_refuses(over):
    L = _lib_hostio()
    assert L.oc_pack_host(*_pack_args(**over)) != 0
    assert L.oc_hostio_last_error() == b"oc_pack_host: bad argument"
    assert L.oc_pack_host_tiled(*_pack_args(**over)) != 0
    assert L.oc_hostio_last_error() == b"oc_pack_host_tiled: bad argument"


def test_tiled_pack_refuses_a_plan_with_unnamed_columns_and_blocks_wider_than_its_lds():
    L = _lib_hostio()
    for over in (dict(w8=18), dict(w64=7), dict(F=30)):              # w64 + w32 + w8 != F
        assert L.oc_pack_host_tiled(*_pack_args(**over)) != 0
        msg = L.oc_hostio_last_error()
        assert msg.startswith(b"oc_pack_host_tiled: ") and b"equal F" in msg and b"launch" not in msg
    # one env's row of 4 062 int64 columns and 24 bytes of vectors is 32 520 bytes; the kernel stages 32 768 - 256
    assert L.oc_pack_host_tiled(*_pack_args(F=4062, w64=4062, w32=0, w8=0)) != 0
    msg = L.oc_hostio_last_error()
    assert msg.startswith(b"oc_pack_host_tiled: ") and b"too wide" in msg
    # an empty batch is accepted and launches nothing
    assert L.oc_pack_host_tiled(*_pack_args(n=0)) == 0


def test_tile_is_a_positive_multiple_of_the_wave():
    L = _lib_hostio()
    t = L.oc_pack_host_tile()
    assert t > 0 and t % 64 == 0


def test_alloc_and_free_check_their_arguments_first():
    L = _lib_hostio()
    host, dev = ctypes.c_void_p(), ctypes.c_void_p()
    for args in ((0, ctypes.byref(host), ctypes.byref(dev)), (-4096, ctypes.byref(host), ctypes.byref(dev)),
                 (4096, None, ctypes.byref(dev)), (4096, ctypes.byref(host), None)):
        assert L.oc_hostio_alloc(*args) != 0
        assert L.oc_hostio_last_error() == b"oc_hostio_alloc: bad argument"
    assert host.value is None and dev.value is None
    assert L.oc_hostio_free(None) != 0
    assert L.oc_hostio_last_error() == b"oc_hostio_free: bad argument"


def test_a_valid_alloc_without_a_device_fails_with_the_runtimes_text():
    L = _lib_hostio()
    host, dev = ctypes.c_void_p(0x10), ctypes.c_void_p(0x10)
    rc = L.oc_hostio_alloc(4096, ctypes.byref(host), ctypes.byref(dev))
    if torch.cuda.is_available():                                  # with a device it simply works
        assert rc == 0 and host.value and dev.value
        assert L.oc_hostio_free(host) == 0
        return
    assert rc != 0 and rc != -1                                    # the runtime's code, not the argument check's
    msg = L.oc_hostio_last_error()
    assert msg.startswith(b"oc_hostio_alloc: hipHostMalloc: ") and len(msg) > len(b"oc_hostio_alloc: hipHostMalloc: ")
    assert host.value is None and dev.value is None                # nothing is handed out


def test_hostio_kernels_have_no_private_segment(tmp_path):
    from gym_comm_amd import build
    if not all(os.path.exists(TOOLS + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    so = build.build_lib("hostio")
    fat, co = str(tmp_path / "f.bin"), str(tmp_path / "k.co")
    subprocess.run([TOOLS + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
    subprocess.run([TOOLS + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
    notes = subprocess.run([TOOLS + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    names = re.findall(r"\.name:\s+(\S+)", notes)
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
    assert len([k for k in names if "k_pack_host_tiled" in k]) == 3          # one per row type
    assert len(sizes) == 6 and max(sizes) == 0, sizes                        # and the three of k_pack_host


@pytest.mark.parametrize("mode", ["bogus", "Mapped", "", None, 1])
def test_unknown_host_io_raises_before_the_batch_is_constructed(monkeypatch, mode):
    from gym_comm_amd.batched import BatchedOvercooked
    from gym_comm_amd.vec_env import OvercookedVecEnv
    seen = []

    def init(self, level, **kw):
        seen.append((level, kw))
        raise AssertionError("the batch was constructed")
    monkeypatch.setattr(BatchedOvercooked, "__init__", init)
    arg = SimpleNamespace(level="open-divider_salad", num_agents=2, max_num_timesteps=30, ego_config={},
                          partner_config={}, num_communication=3, communication_on=True, ego_led=False, fow_radius=1)
    with pytest.raises(ValueError) as e:
        OvercookedVecEnv(arg, 64, host_io=mode)
    assert "host_io" in str(e.value) and "mapped" in str(e.value)
    assert not seen
    for ok in ("copy", "mapped"):                   # the two modes get as far as the constructor
        with pytest.raises(AssertionError):
            OvercookedVecEnv(arg, 64, host_io=ok)
    assert len(seen) == 2
