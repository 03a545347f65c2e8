"""Map sets (include/oc_hip.h: oc_mapset_*; BatchedOvercooked.from_maps), the part that needs no GPU:
the C ABI's new names and their ctypes mirror, from_maps' argument validation -- all of it before
the batch is constructed, i.e. before any GPU call -- and which built libraries hold the set kernels
(structure libraries do, level libraries do not), read from the code objects' notes."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = "/opt/rocm/lib/llvm/bin/"
NAMES = ["oc_mapset_create", "oc_mapset_destroy", "oc_mapset_reset", "oc_mapset_obs", "oc_mapset_multi_step",
         "oc_mapset_multi_step_waves"]
TOMATO = ["open-divider_tomato", "partial-divider_tomato", "full-divider_tomato"]


def test_new_names_are_in_the_header_and_in_the_loader():
    from gym_comm_amd import _lib
    with open(os.path.join(ROOT, "include", "oc_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"OC_API\s+\w+\s+%s\(" % name, header), name
        assert name in _lib.LIBS["hip"].protos, name
    assert re.search(r"#define OC_ABI_VERSION 6\b", header)           # additive: the version stays
    # the same arguments as the single-level forms plus group_map
    protos = _lib.LIBS["hip"].protos
    for single, many in (("oc_reset", "oc_mapset_reset"), ("oc_obs", "oc_mapset_obs"),
                         ("oc_multi_step", "oc_mapset_multi_step")):
        assert len(protos[many][1]) == len(protos[single][1]) + 1, many
    L = _lib.load()
    for name in NAMES:
        getattr(L, name)


@pytest.fixture
def no_batch(monkeypatch):
    """from_maps with the constructor replaced: a call that gets that far records its arguments
    instead of touching a device."""
    from gym_comm_amd.batched import BatchedOvercooked
    seen = []

    def init(self, level, **kw):
        seen.append((level, kw))
    monkeypatch.setattr(BatchedOvercooked, "__init__", init)
    return BatchedOvercooked, seen


def test_structure_mismatch_names_both_levels(no_batch):
    B, seen = no_batch
    with pytest.raises(ValueError) as e:
        B.from_maps(["open-divider_tomato", "full-divider_salad"], num_envs=128)
    assert "open-divider_tomato" in str(e.value) and "full-divider_salad" in str(e.value)
    with pytest.raises(ValueError) as e:       # the same recipes, another border kind and item multiset
        B.from_maps(["open-divider_tomato", "random-open-divider_tomato"], num_envs=128)
    assert "open-divider_tomato" in str(e.value) and "random-open-divider_tomato" in str(e.value)
    assert not seen


@pytest.mark.parametrize("kw", [
    dict(num_envs=229, group_map=[0, 1, 3, 1]),             # a value past the last map
    dict(num_envs=229, group_map=[0, -1, 2, 1]),
    dict(num_envs=229, group_map=[0, 1, 2]),                # one group short
    dict(num_envs=229, group_map=[0, 1, 2, 1, 0]),          # one too many
    dict(num_envs=229, group_map=[[0, 1], [2, 1]]),
    dict(num_envs=229, group_map=[0.0, 1.0, 2.0, 1.0]),
    dict(envs_per_map=[64, 100, 64]),                       # a partial group that is not the batch's last
    dict(envs_per_map=[63, 64, 64]),
    dict(envs_per_map=[64, 64]),                            # one count per level
    dict(envs_per_map=[64, 64, 64], group_map=[0, 1, 2]),   # both
    dict(envs_per_map=[64, 64, 64], num_envs=200),
    dict(),                                                 # no batch size at all
    dict(num_envs=0),
    dict(num_envs=128, policy=((0, 0, 0, None),) * 2),      # the fused policies
    dict(num_envs=128, communication_on=False),             # not the standard wrapper configuration
    dict(num_envs=128, ego_config={"BLIND": True}),
    dict(num_envs=128, play=True),
    dict(num_envs=128, num_agents=3),
])
def test_bad_arguments_raise_before_any_gpu_call(no_batch, kw):
    B, seen = no_batch
    with pytest.raises(ValueError):
        B.from_maps(TOMATO, **kw)
    assert not seen


def test_valid_arguments_reach_the_constructor_with_the_assignment(no_batch):
    B, seen = no_batch
    B.from_maps(TOMATO, num_envs=229, group_map=[0, 1, 2, 1], num_communication=3)
    B.from_maps(TOMATO, envs_per_map=[128, 0, 37])
    B.from_maps(TOMATO, num_envs=300)
    (lv, a), (_, b), (_, c) = seen
    assert lv.name == "open-divider_tomato" and a["num_envs"] == 229 and a["num_communication"] == 3
    assert [m.name for m in a["_maps"][0]] == TOMATO
    assert a["_maps"][1].dtype == np.int32 and a["_maps"][1].tolist() == [0, 1, 2, 1]
    assert b["num_envs"] == 165 and b["_maps"][1].tolist() == [0, 0, 2]       # the last group holds 37 envs
    assert c["_maps"][1].tolist() == [0, 1, 2, 0, 1]                          # dealt round-robin


def _kernel_names(so, tmp_path):
    from gym_comm_amd import build
    fat, co = str(tmp_path / "f.bin"), str(tmp_path / "k.co")
    subprocess.run([TOOLS + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, so], check=True)
    subprocess.run([TOOLS + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--" + build.ARCH, "--output=" + co], check=True)
    notes = subprocess.run([TOOLS + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    os.remove(fat), os.remove(co)
    return re.findall(r"\.name:\s+(\S+)", notes)


def test_structure_library_holds_the_set_kernels_and_level_library_none(tmp_path):
    from gym_comm_amd import compiler, specialize
    if not all(os.path.exists(TOOLS + t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("llvm binary tools not available")
    lv = compiler.compile_level("open-divider_tomato", 2, 500)
    structure = specialize.ensure(lv.blob, geometry=False, compile=False)
    level = specialize.ensure(lv.blob, geometry=True, compile=False)
    assert structure and level, "build() makes both libraries of open-divider_tomato x2"
    names = _kernel_names(structure, tmp_path)
    # k_mapset_step<M, OT, DUP, XO, SP>: three row types x XO 0 / 1 x one wave / four waves
    step = sorted(re.search(r"k_mapset_stepILi4ELi(\d)ELb0ELi(\d)ELi(\d)EE", k).groups()
                  for k in names if "k_mapset_step" in k)
    assert step == sorted((ot, xo, sp) for ot in "012" for xo in "01" for sp in "14")
    assert len([k for k in names if "k_mapset_obs" in k]) == 3
    assert len([k for k in names if "k_mapset_reset" in k]) == 1
    assert not any("k_multi_step" in k for k in names if "k_mapset" in k)      # (names other tests parse)
    assert not [k for k in _kernel_names(level, tmp_path) if "k_mapset" in k]
    assert not [k for k in _kernel_names(os.path.join(ROOT, "gym-comm_amd", "csrc", "liboc_hip.so"), tmp_path)
                if "k_mapset" in k]
