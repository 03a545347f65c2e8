"""ctypes loader for the native libraries: liboc_hip.so (include/oc_hip.h) and its per-level
specialisations, liboc_policy.so, liboc_hostio.so and liboc_rollout.so.

There is no CPU fallback: if a library cannot be loaded, or a call fails, this
raises.  (The CPU oracle under oracle/ is test infrastructure and is never used here.)
"""
import collections
import contextlib
import ctypes
import os

import torch

from . import build as _build

_I32P = ctypes.POINTER(ctypes.c_int32)


class ObsCfg(ctypes.Structure):
    _fields_ = [("fow_radius", ctypes.c_int32), ("blind_mask", ctypes.c_int32),
                ("num_comm", ctypes.c_int32), ("obs_int8", ctypes.c_int32)]


class WrapCfg(ctypes.Structure):
    _fields_ = [("obs", ObsCfg), ("communication_on", ctypes.c_int32),
                ("ego_led", ctypes.c_int32), ("ego_agent_idx", ctypes.c_int32),
                ("can_move_mask", ctypes.c_int32)]


class StepPolicy(ctypes.Structure):
    """oc_step_policy (include/oc_hip.h): one player's packed MLP for oc_step_opts.policy."""
    _fields_ = [("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p), ("rng", ctypes.c_void_p)]


class StepOpts(ctypes.Structure):
    """oc_step_opts (include/oc_hip.h): optional device pointers of oc_multi_step."""
    _fields_ = [("ep_return", ctypes.c_void_p), ("ep_length", ctypes.c_void_p),
                ("ego_pairs", ctypes.c_void_p), ("alt_pairs", ctypes.c_void_p),
                ("alt_rng", ctypes.c_void_p), ("alt_played", ctypes.c_void_p),
                ("pairs_int64", ctypes.c_int32), ("waves_per_64", ctypes.c_int32),
                ("policy", ctypes.POINTER(StepPolicy))]


class PolicyPlayer(ctypes.Structure):
    """oc_policy_player (include/oc_policy.h)."""
    _fields_ = [("obs", ctypes.c_void_p), ("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p),
                ("b2", ctypes.c_void_p), ("rng", ctypes.c_void_p), ("pairs", ctypes.c_void_p),
                ("logits", ctypes.c_void_p)]


class PolicyAcPlayer(ctypes.Structure):
    """oc_policy_ac_player (include/oc_policy.h)."""
    _fields_ = [("p", PolicyPlayer), ("given", ctypes.c_void_p), ("move_row", ctypes.c_void_p),
                ("comm_row", ctypes.c_void_p), ("log_prob", ctypes.c_void_p), ("value", ctypes.c_void_p)]


class PolicyLstmPlayer(ctypes.Structure):
    """oc_policy_lstm_player (include/oc_policy.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "gates", "head", "head_bias", "h_in", "c_in", "h_out", "c_out", "episode_start", "rng", "given",
                 "pairs", "move_row", "comm_row", "log_prob", "value", "logits")]


class PpoCfg(ctypes.Structure):
    """oc_ppo_cfg (include/oc_policy.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "timestep", "actions", "log_probs", "advantages", "returns")] + \
               [("n", ctypes.c_int64), ("T", ctypes.c_int32), ("F", ctypes.c_int32), ("C", ctypes.c_int32),
                ("obs_type", ctypes.c_int32)] + \
               [(name, ctypes.c_void_p) for name in
                ("w1", "w2", "b2", "w2t", "p_w1", "p_wt", "p_b1", "p_w2", "p_b2", "p_wv", "p_bv", "m", "v", "step",
                 "grad", "scratch", "stats", "hyper")] + \
               [(name, ctypes.c_float) for name in ("ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps")] + \
               [("max_groups", ctypes.c_int32), ("lp_out", ctypes.c_void_p), ("v_out", ctypes.c_void_p)]


class RppoCfg(ctypes.Structure):
    """oc_rppo_cfg (include/oc_policy.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "timestep", "actions", "log_probs", "advantages", "returns", "episode_starts", "h0", "c0")] + \
               [("n", ctypes.c_int64), ("T", ctypes.c_int32), ("F", ctypes.c_int32), ("C", ctypes.c_int32),
                ("obs_type", ctypes.c_int32)] + \
               [(name, ctypes.c_void_p) for name in
                ("gates", "head", "head_bias", "bwd", "p_wx", "p_wt", "p_b", "p_wh", "p_w2", "p_b2", "p_wv", "p_bv",
                 "m", "v", "step", "grad", "scratch", "stats", "hyper")] + \
               [(name, ctypes.c_float) for name in ("ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps")] + \
               [("max_groups", ctypes.c_int32), ("lp_out", ctypes.c_void_p), ("v_out", ctypes.c_void_p)]


class WindowSrc(ctypes.Structure):
    """oc_window_src (include/oc_policy.h): a sink's tensors and the states recorded where its windows begin."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "timestep", "actions", "log_probs", "advantages", "returns", "episode_starts", "values",
                 "states")] + \
               [("n", ctypes.c_int64), ("T", ctypes.c_int32), ("W", ctypes.c_int32), ("F", ctypes.c_int32),
                ("obs_type", ctypes.c_int32)]


class WindowBatch(ctypes.Structure):
    """oc_window_batch (include/oc_policy.h): a minibatch of windows laid out as a sink of W slots and E envs."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "timestep", "actions", "log_probs", "advantages", "returns", "episode_starts", "values",
                 "h0", "c0")]


class PpoTrain(ctypes.Structure):
    """oc_ppo_train (include/oc_policy.h): the train sequence's device state."""
    _fields_ = [(name, ctypes.c_void_p) for name in ("values", "hyper_ext", "ctl", "acc")]


# oc_ppo_train's word indices (OC_PPO_CTL_* / OC_PPO_ACC_* of include/oc_policy.h)
PPO_CTL = {"stop": 0, "epoch": 1, "updates": 2, "epochs": 3, "error": 4, "words": 8}
PPO_ACC = {"epoch_kl": 0, "epoch_count": 1, "sums": 2, "words": 8}


class RolloutBuf(ctypes.Structure):
    """oc_rollout_buf (include/oc_rollout.h)."""
    _fields_ = [(name, ctypes.c_void_p) for name in
                ("obs", "timestep", "actions", "log_probs", "values", "episode_starts", "rewards", "dones",
                 "pos", "last", "count", "ticket", "advantages", "returns")] + \
               [("n", ctypes.c_int64), ("T", ctypes.c_int32), ("F", ctypes.c_int32), ("obs_type", ctypes.c_int32)]


class OcError(RuntimeError):
    pass


# One record per native library (built by build.LIBS[name]): the environment variable that overrides
# its path, its ABI-version function and the version this loader was written for (the header's
# OC_*ABI_VERSION), its last-error function, and its prototypes, symbol -> (restype, argtypes);
# argtypes None = left undeclared (no parameters).
Lib = collections.namedtuple("Lib", "env abi_fn abi_version last_error protos")


def _libs_table():
    cint, cstr, vp, fp = ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    i32, i64, u32, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.POINTER
    bp = P(RolloutBuf)
    multi_step = [vp, vp, vp, vp, P(WrapCfg), vp, vp, vp, vp, vp, i32, vp, vp, vp, P(StepOpts), i64]
    return {
        "hip": Lib("OC_HIP_LIB", "oc_abi_version", 6, "oc_last_error", {
            "oc_abi_version": (cint, None),
            "oc_last_error": (cstr, None),
            "oc_is_specialized": (cint, None),
            "oc_level_create": (cint, [_I32P, i32, P(vp)]),
            "oc_level_destroy": (cint, [vp]),
            "oc_level_spec_source": (cint, [_I32P, i32, i32, cstr, i32]),
            "oc_level_subtask_info": (cint, [_I32P, i32, _I32P, _I32P, _I32P]),
            "oc_metrics_slots": (i64, [i64]),
            "oc_state_words": (i32, [vp]),
            "oc_obs_rows": (i32, [vp, i32]),
            "oc_image_words": (i32, [vp]),
            "oc_reset": (cint, [vp, vp, vp, vp, vp, i64, vp]),
            "oc_step": (cint, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, vp]),
            "oc_obs": (cint, [vp, vp, vp, P(ObsCfg), vp, vp, i64, vp]),
            "oc_obs_image": (cint, [vp, vp, i32, vp, vp, i64, vp]),
            "oc_multi_step": (cint, multi_step + [vp]),
            "oc_multi_step_waves": (i32, [i64, i32, i32]),
            "oc_multi_step_lanes": (i32, [i64, i32, i32]),
            "oc_random_actions": (cint, [vp, vp, vp, i32, i64, vp]),
            "oc_timeline_begin": (cint, [vp, i64, i64]),
            "oc_multi_step_prepare": (cint, multi_step + [P(vp)]),
            "oc_call_launch": (cint, [vp, vp, i32, vp]),
            "oc_call_destroy": (cint, [vp]),
            # map sets (structure libraries): the set and the device group_map in the level's place
            "oc_mapset_create": (cint, [P(_I32P), _I32P, i32, P(vp)]),
            "oc_mapset_destroy": (cint, [vp]),
            "oc_mapset_reset": (cint, [vp, vp, vp, vp, vp, vp, i64, vp]),
            "oc_mapset_obs": (cint, [vp, vp, vp, vp, P(ObsCfg), vp, vp, i64, vp]),
            "oc_mapset_multi_step": (cint, [vp] + multi_step + [vp]),
            "oc_mapset_multi_step_waves": (i32, [i64, i32, i32]),
        }),
        "policy": Lib("OC_POLICY_LIB", "oc_policy_abi_version", 1, "oc_policy_last_error", {
            "oc_policy_abi_version": (cint, None),
            "oc_policy_last_error": (cstr, None),
            "oc_policy_ksteps": (i32, [i32]),
            "oc_policy_pack_w1": (cint, [fp, fp, fp, i32, vp]),
            "oc_policy_pack_w2": (cint, [fp, i32, vp]),
            "oc_policy_pack_b2": (cint, [fp, fp, i32, fp]),
            "oc_policy_mlp": (cint, [P(PolicyPlayer), i32, vp, i32, i32, i32, i64, vp]),
            "oc_policy_pack_w2v": (cint, [fp, fp, i32, vp]),
            "oc_policy_pack_b2v": (cint, [fp, fp, fp, fp, i32, fp]),
            "oc_policy_mlp_ac": (cint, [P(PolicyAcPlayer), i32, vp, i32, i32, i32, i64, vp]),
            # the PPO update of the actor-critic form
            "oc_policy_pack_w2t": (cint, [fp, fp, i32, fp]),
            "oc_policy_ppo_plan": (cint, [i32, i32, i32, i32, _I32P]),
            "oc_policy_ppo_update": (cint, [P(PpoCfg), vp, i32, vp]),
            "oc_policy_ppo_grad": (cint, [P(PpoCfg), vp, i32, vp]),
            # the train sequence: device shuffle, KL stop, value clipping, accumulated statistics
            "oc_policy_ppo_perm_host": (cint, [u32, i32, i32, _I32P]),
            "oc_policy_ppo_train_begin": (cint, [P(PpoTrain), vp]),
            "oc_policy_ppo_epoch_begin": (cint, [P(PpoTrain), vp, i32, i32, u32, vp]),
            "oc_policy_ppo_train_step": (cint, [P(PpoCfg), P(PpoTrain), vp, i32, vp]),
            # the recurrent seat: an LSTM actor-critic step
            "oc_policy_lstm_ksteps": (i32, [i32]),
            "oc_policy_lstm_pack_gates": (cint, [fp, fp, fp, fp, i32, vp]),
            "oc_policy_lstm_pack_head": (cint, [fp, fp, i32, vp]),
            "oc_policy_lstm_pack_head_bias": (cint, [fp, fp, i32, fp]),
            "oc_policy_lstm_ac": (cint, [P(PolicyLstmPlayer), vp, i32, i32, i32, i64, vp]),
            # windows of a rollout: the state snapshot and the gather of a minibatch of windows
            "oc_policy_window_snapshot": (cint, [vp, i32, i32, vp, vp, vp, i64, vp]),
            "oc_policy_window_gather": (cint, [P(WindowSrc), P(WindowBatch), vp, i32, vp]),
            # the recurrent seat's PPO update
            "oc_policy_rppo_plan": (cint, [i32, i32, i32, i32, i32, P(i64)]),
            "oc_policy_rppo_pack_bwd_elems": (i32, None),
            "oc_policy_rppo_pack_bwd": (cint, [fp, fp, fp, i32, fp]),
            "oc_policy_rppo_update": (cint, [P(RppoCfg), vp, i32, vp]),
            "oc_policy_rppo_grad": (cint, [P(RppoCfg), vp, i32, vp]),
            # ... and its step of the train sequence (between oc_policy_ppo_train_begin / _epoch_begin)
            "oc_policy_recurrent_train_step": (cint, [P(RppoCfg), P(PpoTrain), vp, i32, vp]),
        }),
        "hostio": Lib("OC_HOSTIO_LIB", "oc_hostio_abi_version", 1, "oc_hostio_last_error", {
            "oc_hostio_abi_version": (cint, None),
            "oc_hostio_last_error": (cstr, None),
            "oc_pack_host_bytes": (i64, [i32, i32, i32, i32, i32, i32, i32, i64]),
            "oc_pack_host": (cint, [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
            # host-mapped I/O: the same pack for an `out` across PCIe, and the mapped allocation
            "oc_pack_host_tiled": (cint, [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
            "oc_pack_host_tile": (cint, None),
            "oc_hostio_alloc": (cint, [i64, P(vp), P(vp)]),
            "oc_hostio_free": (cint, [vp]),
        }),
        "rollout": Lib("OC_ROLLOUT_LIB", "oc_rollout_abi_version", 1, "oc_rollout_last_error", {
            "oc_rollout_abi_version": (cint, None),
            "oc_rollout_last_error": (cstr, None),
            "oc_rollout_add": (cint, [bp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "oc_rollout_add_plan": (cint, [bp, P(i32)]),
            "oc_rollout_add_reward": (cint, [bp, vp, vp, vp]),
            "oc_rollout_gae": (cint, [bp, vp, vp, ctypes.c_double, ctypes.c_double, vp]),
        }),
    }


LIBS = _libs_table()
_libs = {}
_hip_preloaded = False


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).
    Our library must bind to THAT runtime instance -- device pointers and streams come
    from torch -- so make sure it is the one already loaded when liboc_hip.so resolves
    its libamdhip64.so.7 dependency."""
    global _hip_preloaded
    if _hip_preloaded:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    _hip_preloaded = True


def load(path=None, lib="hip"):
    """Load (once per path) and type a library of LIBS.  Default path: the one build.py builds;
    for "hip" a per-level specialisation's path may be given instead."""
    rec = LIBS[lib]
    default = _build.LIBS[lib].lib
    path = os.path.abspath(path or os.environ.get(rec.env) or default)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise OcError(
            "HIP extension %s not built: run `python -c 'import __graft_entry__ as g; g.build()'`"
            " (there is no CPU fallback)" % path)
    _preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in rec.protos.items():
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    if getattr(L, rec.abi_fn)() != rec.abi_version:
        raise OcError("%s ABI version mismatch" % os.path.basename(default))
    L._oc_last_error = getattr(L, rec.last_error)
    L._oc_path = path
    _libs[path] = L
    return L


def check(rc, what, lib=None):
    """Raise OcError with the library's own last-error text unless rc is 0."""
    if rc != 0:
        msg = (lib or load())._oc_last_error()
        raise OcError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def raw_stream(dev):
    """hipStream_t of torch's current stream on device index `dev`, as an int."""
    try:
        return torch._C._cuda_getCurrentRawStream(dev)      # ~0.3 us
    except AttributeError:                                 # older/newer torch
        return torch.cuda.current_stream(dev).cuda_stream


def on_device(dev):
    """Context in which device index `dev` is current (kernels must be launched with their tensors'
    device current; one process per GPU is the normal case and costs nothing here)."""
    if torch.cuda.current_device() == dev:
        return contextlib.nullcontext()
    return torch.cuda.device(dev)


def call(L, name, dev, *args, stream=True):
    """Entry point `name` of library L with device `dev` current -- followed, for a launching entry
    point, by torch's current raw stream on it as the last argument -- and its return code checked."""
    with on_device(dev):
        rc = getattr(L, name)(*args, raw_stream(dev)) if stream else getattr(L, name)(*args)
    check(rc, name, L)


def subtask_info(blob, lib=None):
    """(slot, goal_index, dup) of a level blob (include/oc_hip.h: oc_level_subtask_info): where the
    state tensor keeps the bits of the blob's subtask s.  Host only."""
    import numpy as np
    L = lib or load()
    blob = np.ascontiguousarray(blob, dtype=np.int32)
    S = int(blob[6])
    slot, gi = np.zeros(S, np.int32), np.zeros(S, np.int32)
    dup = ctypes.c_int32()
    check(L.oc_level_subtask_info(blob.ctypes.data_as(_I32P), int(blob.size), slot.ctypes.data_as(_I32P),
                                  gi.ctypes.data_as(_I32P), ctypes.byref(dup)), "oc_level_subtask_info", L)
    return slot.tolist(), gi.tolist(), bool(dup.value)
