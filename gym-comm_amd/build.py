"""Build liboc_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

hipcc cross-compiles without a GPU; the built library travels to the GPU box with the
repo snapshot.  ``-ffp-contract=off``: reward shaping must reproduce CPython's fp64
arithmetic bit for bit, so no fused multiply-adds may be formed.
"""
import collections
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
ARCH = "gfx950"
# the stepper (include/oc_hip.h).  SOURCES / HEADERS / LOCAL_HEADERS / FLAGS are also what the
# specialised builds compile (specialize.py) and what their cache key hashes
SOURCES = ["oc_kernels.hip"]
HEADERS = ["oc_hip.h", "oc_level.h"]          # include/: what SOURCES include
# csrc/: the stepper's host half and its kernels, and the policy's device code (shared with oc_policy.hip)
LOCAL_HEADERS = ["oc_level_host.h", "oc_step_device.h", "oc_policy_device.h"]
LIB = os.path.join(CSRC, "liboc_hip.so")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
         "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
         # leading scalar kernel arguments (k_multi_step) arrive in SGPRs at wave launch
         "-mllvm", "-amdgpu-kernarg-preload-count=9"]
# experiment switches (e.g. OC_HIP_EXTRA_FLAGS=-DOC_TABLES_IN_LDS); they enter the
# specialisation cache key, so variants never collide
FLAGS += [f for f in os.environ.get("OC_HIP_EXTRA_FLAGS", "").split() if f]
_PLAIN_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]

Lib = collections.namedtuple("Lib", "sources headers local_headers flags lib")
# one record per shared object: sources and local headers under csrc/, public headers under include/
LIBS = {
    "hip": Lib(SOURCES, HEADERS, LOCAL_HEADERS, FLAGS, LIB),
    # the policy library (include/oc_policy.h): its own translation unit and shared object, so that
    # the stepper's specialised builds neither contain nor depend on it
    # (oc_policy_ppo.hip: the PPO update, a second translation unit and code object of the same library;
    # oc_policy_lstm.hip: the recurrent seat, a third; oc_policy_window.hip: the window snapshot and gather;
    # oc_policy_rppo.hip: the recurrent update; oc_policy_rtrain.hip: the recurrent learner's step of the train sequence;
    # oc_policy_train.hip: the train sequence, kept LAST: the code objects keep their order)
    "policy": Lib(["oc_policy.hip", "oc_policy_ppo.hip", "oc_policy_lstm.hip", "oc_policy_window.hip", "oc_policy_rppo.hip",
                   "oc_policy_rtrain.hip", "oc_policy_train.hip"],
                  ["oc_policy.h"],
                  ["oc_policy_device.h", "oc_policy_ac_device.h", "oc_policy_ppo_device.h", "oc_policy_layout.h",
                   "oc_policy_fail.h", "oc_policy_shuffle.h", "oc_policy_rppo_device.h", "oc_policy_rppo_host.h"],
                  _PLAIN_FLAGS,
                  os.path.join(CSRC, "liboc_policy.so")),
    # the host-I/O library (include/oc_hostio.h): the numpy boundary's pack-for-PCIe kernel
    "hostio": Lib(["oc_hostio.hip"], ["oc_hostio.h"], [], _PLAIN_FLAGS, os.path.join(CSRC, "liboc_hostio.so")),
    # the rollout-buffer library (include/oc_rollout.h): one-launch recording and the GAE kernel, whose
    # float32 chain must reproduce stable-baselines3's operation order bit for bit: no contraction
    "rollout": Lib(["oc_rollout.hip"], ["oc_rollout.h"], [], _PLAIN_FLAGS + ["-ffp-contract=off", "-fno-fast-math"],
                   os.path.join(CSRC, "liboc_rollout.so")),
}


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC=)")


def needs_build(rec=LIBS["hip"]):
    if not os.path.exists(rec.lib):
        return True
    deps = [os.path.join(CSRC, s) for s in list(rec.sources) + list(rec.local_headers)]
    inc = os.path.join(CSRC, "..", "..", "include")
    deps += [os.path.join(inc, f) for f in rec.headers]
    return os.path.getmtime(rec.lib) < max(os.path.getmtime(d) for d in deps)


def _compile(lib, sources, flags, verbose):
    cmd = [hipcc_path(), "--offload-arch=" + ARCH] + list(flags)
    tmp = "%s.%d.tmp" % (lib, os.getpid())        # concurrent builders never share a temporary
    cmd += [os.path.join(CSRC, s) for s in sources] + ["-o", tmp]
    if verbose:
        print(" ".join(cmd), flush=True)
    env = {k: v for k, v in os.environ.items()
           if k != "LD_PRELOAD" and not k.startswith(("ROCP_", "ROCPROF", "ROCTRACER", "HSA_TOOLS_LIB"))}
    try:
        subprocess.check_call(cmd, env=env)
        os.replace(tmp, lib)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return lib


def build_lib(name, force=False, verbose=False, extra_flags=()):
    """Compile shared object `name` of LIBS into csrc/.  Returns the library path."""
    rec = LIBS[name]
    if not force and not needs_build(rec):
        return rec.lib
    return _compile(rec.lib, rec.sources, list(rec.flags) + list(extra_flags), verbose)


def build(force=False, verbose=False, extra_flags=()):
    """Compile the stepper into csrc/liboc_hip.so.  Returns the library path."""
    return build_lib("hip", force, verbose, extra_flags)


if __name__ == "__main__":
    for name in LIBS:
        print(build_lib(name, force=True, verbose=True))
