"""BatchedOvercooked: N independent Overcooked envs of one level -- or, ``from_maps``, of several
maps of one level structure -- on one MI355X.

Host side of the hot path: owns the PyTorch-ROCm tensors (env-major int32 SoA) and calls
the hand-written HIP kernels of liboc_hip.so through the C ABI (include/oc_hip.h) with
raw device pointers on torch's current stream.  No compute happens in Python or torch.

Mirrors, batched:
  gym_cooking.envs.OvercookedEnvironment.step/reset    (overcooked_environment.py:180-241)
  gym_comm.envs.OvercookedMultiEnv.multi_step/multi_reset/get_observation2
                                                       (overcooked_env.py:105-297)
"""
import ctypes
import functools
from typing import Optional

import numpy as np
import torch

from . import _lib, compiler, specialize
from .state import unpack_state

OBS_KEYS = ["object_encodings_x", "object_encodings_y", "state_encodings", "is_hidden",
            "completed_subtasks", "agent1_location", "agent2_location", "agent_is_holding",
            "agent1_comm", "agent2_comm"]
# obs_type of the C ABI (include/oc_hip.h, oc_policy.h, oc_hostio.h, oc_rollout.h): the dtype of observation rows
OBS_TYPE = {torch.int32: 0, torch.int8: 1, torch.float32: 2}


def pcg32_seed_states(seed, shape, device="cpu"):
    """int32 `shape` tensor of seeded PCG32 states (uint32 bit patterns below 2^31) on `device`."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randint(0, 2 ** 31 - 1, tuple(shape), generator=g, dtype=torch.int64).to(torch.int32).to(device)


def obs_layout(S, C):
    """Row ranges of each observation key inside the [F] axis (F = 22 + S + 2C)."""
    sizes = [4, 4, 4, 4, S, 2, 2, 2, C, C]
    out, r = {}, 0
    for k, s in zip(OBS_KEYS, sizes):
        out[k] = (r, r + s)
        r += s
    return out


def nominal_placement(levels, group_map, n):
    """int32 [M][n]: every env's item start cells (x | y<<4, world order) as its OWN map compiled them --
    the first Counters of that map for the scattered items.  ``levels``: the compiled maps of a set (one
    for a single level); ``group_map``: a map index per group of 64 envs, or None for map 0 everywhere."""
    cols = np.array([lv.pack_placement([(x, y) for _, x, y in lv.items]) for lv in levels], np.int32)
    cols = cols.reshape(len(levels), -1)
    if group_map is None:
        env_map = np.zeros(int(n), np.int64)
    else:
        env_map = np.asarray(group_map, np.int64)[np.arange(int(n)) // 64]
    return np.ascontiguousarray(cols[env_map].T)


class PreparedStep:
    """A fused step with every argument but the ego's pairs fixed (``BatchedOvercooked.prepare_multi_step``).
    Calling it -- or its ``launch`` attribute, which saves a frame -- is ``launch(ego_pairs_ptr_or_None,
    pairs_int64)``.  ``close()`` destroys the native ``oc_call`` behind it, once (a map set's form has
    none: a no-op there); the batch lists the open ones in ``live`` and closes what is left when it goes.
    The handle holds the env's tensors by ADDRESS: they must not be rebound while a prepared step is alive."""
    closed = False

    def __init__(self, launch, lib=None, handle=None, live=None):
        self.launch, self._lib, self._handle, self._live = launch, lib, handle, live
        if handle is not None and live is not None:
            live.append(self)

    def __call__(self, ego_pairs_ptr=None, pairs_int64=False):
        self.launch(ego_pairs_ptr, pairs_int64)

    @staticmethod
    def _refuse(ego_pairs_ptr=None, pairs_int64=False):
        raise RuntimeError("this prepared step was closed")

    def close(self):
        handle, self._handle, self.launch, self.closed = self._handle, None, self._refuse, True
        if handle is not None:
            if self._live is not None:
                self._live.remove(self)
            self._lib.oc_call_destroy(handle)


class BatchedOvercooked:
    def __init__(self, level, num_agents=2, num_envs=4096, max_num_timesteps=100,
                 ego_config=None, partner_config=None, num_communication=2,
                 communication_on=True, ego_led=False, fow_radius=2, ego_agent_idx=0,
                 device="cuda", subtask_order=None, placements=None, level_dir=None,
                 max_num_subtasks=14, auto_reset=True, track_metrics=True, specialize_level="auto",
                 seed=0, placement_mode="rng", obs_dtype=torch.int32, episode_stats=False, play=False,
                 waves_per_64=0, _maps=None):
        cfg = {"ALLERGIC": False, "BLIND": False, "CAN_MOVE": True}   # missing CAN_MOVE = True
        self.ego_config = dict(cfg, **(ego_config or {}))
        self.partner_config = dict(cfg, **(partner_config or {}))
        # a map set (from_maps): the compiled levels and the host copy of group_map; `level` is the first
        self.levels, self.group_map_host = _maps if _maps is not None else (None, None)
        if isinstance(level, compiler.CompiledLevel):
            self.level = level
        else:
            self.level = compiler.compile_level(
                level, num_agents, max_num_timesteps, max_num_subtasks,
                ego_allergic=self.ego_config["ALLERGIC"],
                partner_allergic=self.partner_config["ALLERGIC"],
                subtask_order=subtask_order, placements=placements, level_dir=level_dir, play=play)
        lv = self.level
        if not lv.hip_supported:
            raise ValueError("level %r: more than three items of one type, or more than 16 distinct "
                             "merged object names (limits of the packed item words)" % lv.name)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.OcError("BatchedOvercooked needs a ROCm device (got %s); there is no CPU path"
                               % self.device)
        self.n = int(num_envs)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self._dev_index)
        self.A, self.M, self.S = lv.num_agents, lv.num_items, lv.num_subtasks
        self.C = int(num_communication)
        self.auto_reset = bool(auto_reset)
        # launch hint of the fused step (include/oc_hip.h, oc_step_opts.waves_per_64): 0 = the
        # library decides, 1 = one wave per 64 envs, 4 = split launch; results are identical
        if waves_per_64 not in (0, 1, 2, 4):
            raise ValueError("waves_per_64 must be 0 (auto), 1, 2 or 4")
        self.waves_per_64 = int(waves_per_64)
        blob = np.ascontiguousarray(lv.blob, dtype=np.int32)
        # per-level specialised kernels when available (specialize.py), else the generic library;
        # a map set runs on the structure library its maps share
        self.kernel_flavour, self._L = specialize.load_for(blob, "structure" if self.levels else specialize_level)
        # hipStream_t of torch's current stream on this env's device, as an int
        self._raw_stream = functools.partial(_lib.raw_stream, self._dev_index)
        h = ctypes.c_void_p()
        # where the state keeps the bits of subtask s (the library's canonical subtask order)
        self.subtask_slot, self._goal_index, self._dup = _lib.subtask_info(blob, self._L)
        n = self.n
        if self.levels:
            # include/oc_hip.h, map sets: the set and the device group_map take the level's place in
            # every call (self._lead); the entry points carry the same arguments otherwise
            i32p = ctypes.POINTER(ctypes.c_int32)
            blobs = [np.ascontiguousarray(m.blob, dtype=np.int32) for m in self.levels]
            ptrs = (i32p * len(blobs))(*[b.ctypes.data_as(i32p) for b in blobs])
            sizes = np.array([b.size for b in blobs], np.int32)
            self._call("oc_mapset_create", ptrs, sizes.ctypes.data_as(i32p), len(blobs), ctypes.byref(h), stream=False)
            self._h = h
            self.group_map = torch.from_numpy(self.group_map_host).to(self.device)
            self._lead = (self._h, self.group_map.data_ptr())
            self._fn = {k: "oc_mapset_" + k for k in ("reset", "obs", "multi_step", "multi_step_waves")}
            self.W_state = self.A + self.M + 2 + (2 if self._dup else 0)
            self.F = 22 + self.S + 2 * self.C
        else:
            self._call("oc_level_create", blob.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(blob.size),
                       ctypes.byref(h), stream=False)
            self._h = h
            self.group_map = None
            self._lead = (self._h,)
            self._fn = {k: "oc_" + k for k in ("reset", "obs", "multi_step", "multi_step_waves")}
            self.W_state = self._L.oc_state_words(h)
            self.F = self._L.oc_obs_rows(h, self.C)
        if obs_dtype not in OBS_TYPE:
            raise ValueError("obs_dtype must be torch.int32, torch.int8 or torch.float32")
        # Every tensor a step reads or writes is a view of ONE device allocation (each view
        # 256-byte aligned): a host consumer fetches the whole step -- state, rewards, done,
        # observations -- with a single device->host copy (`fetch()`), instead of one per tensor.
        spec = [("state", (self.W_state, n), torch.int32), ("reward", (n,), torch.int32),
                ("done", (n,), torch.int32), ("shaping", (2, n), torch.float64),
                ("comm", (2, n), torch.int32),                  # one-hot(0) (overcooked_env.py:89-91)
                ("obs", (2, self.F, n), obs_dtype), ("timestep", (n,), torch.float64),
                ("shaped_reward", (n,), torch.float64)]
        if episode_stats:           # kept by the fused kernel (include/oc_hip.h: ep_return / ep_length)
            spec += [("ep_return", (n,), torch.float64), ("ep_length", (n,), torch.int32)]
        else:
            self.ep_return = self.ep_length = None
        self._arena_layout, off = {}, 0
        for name, shape, dt in spec:
            nb = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            self._arena_layout[name] = (off, nb, shape, dt)
            off += (nb + 255) // 256 * 256
        self._arena = torch.zeros(max(off, 256), dtype=torch.uint8, device=self.device)
        for name, (o, nb, shape, dt) in self._arena_layout.items():
            setattr(self, name, self._arena[o:o + nb].view(dt).view(shape))
        self.metrics = (torch.zeros((self._L.oc_metrics_slots(n), 8), dtype=torch.int64,
                                    device=self.device) if track_metrics else None)
        self._obs_cfg = _lib.ObsCfg(int(fow_radius),
                                    (1 if self.ego_config["BLIND"] else 0) |
                                    (2 if self.partner_config["BLIND"] else 0), self.C,
                                    OBS_TYPE[obs_dtype])
        self._wrap_cfg = _lib.WrapCfg(self._obs_cfg, int(bool(communication_on)), int(bool(ego_led)),
                                      int(ego_agent_idx),
                                      (1 if self.ego_config["CAN_MOVE"] else 0) |
                                      (2 if self.partner_config["CAN_MOVE"] else 0))
        self._layout = obs_layout(self.S, self.C)
        self._ms_args = None
        self._prepared = []         # the open PreparedStep objects that hold a native handle
        self._policy_arr = None
        self._arena_pinned = None
        self._fetch_plan = None
        # random-* levels: item start cells differ per env and per episode
        self.placement = None
        self.rng = None
        if lv.random_placement:
            if placement_mode == "rng":
                self.rng = pcg32_seed_states(seed, (n,), self.device)
            elif placement_mode == "host":
                # every env starts on its own map's nominal cells (a set's maps differ in their Counters)
                nominal = nominal_placement(self.levels or [lv], self.group_map_host, n)
                self.placement = torch.from_numpy(nominal).to(self.device)
            else:
                raise ValueError("placement_mode must be 'rng' or 'host'")
        self.reset()

    def __del__(self):
        for step in list(getattr(self, "_prepared", [])):
            step.close()
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            (self._L.oc_mapset_destroy if self.levels else self._L.oc_level_destroy)(h)
            self._h = None

    # -- map sets ----------------------------------------------------------------
    @classmethod
    def from_maps(cls, levels, group_map=None, envs_per_map=None, num_envs=None, num_agents=2,
                  max_num_timesteps=100, max_num_subtasks=14, subtask_order=None, level_dir=None, play=False,
                  policy=None, **kw):
        """Envs on DIFFERENT maps of one level structure, stepped by one launch (include/oc_hip.h: map
        sets).  ``levels``: level names or ``CompiledLevel`` objects whose structure (recipes, item
        multiset, 2 agents, border kind) and subtask order are equal; the batch runs on the structure
        library of the first.  Envs are assigned in GROUPS of 64 -- envs 64 g ... 64 g + 63 live on map
        ``group_map[g]`` -- for the life of the batch:
          ``group_map``     one map index per group, ``ceil(num_envs / 64)`` of them, or
          ``envs_per_map``  an env count per map, in map order: multiples of 64 (only the last
                            group of the batch may be partial, so only the last count may not be), or
          neither           the ``num_envs`` envs' groups are dealt round-robin.
        Every other keyword is ``BatchedOvercooked``'s.  Everything is validated here, before any GPU
        call.  The batch has the single-level surface -- ``reset``, ``observe``, ``multi_step`` with rows,
        pairs, the in-kernel partner and episode statistics, ``fetch``, ``get_state`` / ``set_state`` --
        except the base ``step``, ``observe_image`` and the fused policies (``policy=`` raises); a launch
        hint the set kernels have no variant for (``waves_per_64=2``) gets the nearest launch there is;
        ``map_of(i)`` names env i's level and ``read_metrics()`` adds the counters per map."""
        if policy is not None:
            raise ValueError("from_maps: the fused policies (policy=) are not available for map sets")
        if num_agents != 2:
            raise ValueError("from_maps: map sets step exactly 2 agents")
        if not levels:
            raise ValueError("from_maps: need at least one level")
        cfg = {"ALLERGIC": False}
        ego, partner = dict(cfg, **(kw.get("ego_config") or {})), dict(cfg, **(kw.get("partner_config") or {}))
        lvs = [m if isinstance(m, compiler.CompiledLevel) else
               compiler.compile_level(m, 2, max_num_timesteps, max_num_subtasks, ego_allergic=ego["ALLERGIC"],
                                      partner_allergic=partner["ALLERGIC"], subtask_order=subtask_order,
                                      level_dir=level_dir, play=play) for m in levels]
        first = lvs[0]
        want = specialize.spec_header_text(first.blob, geometry=False), _lib.subtask_info(first.blob)
        for m in lvs:
            if not m.hip_supported or m.num_agents != 2:
                raise ValueError("from_maps: level %r is not a 2-agent level the HIP path supports" % m.name)
            got = specialize.spec_header_text(m.blob, geometry=False), _lib.subtask_info(m.blob)
            if got[0] != want[0]:
                raise ValueError("from_maps: levels %r and %r differ in structure (recipes, item multiset, agent "
                                 "count, border kind): a map set needs one structure" % (first.name, m.name))
            if got[1] != want[1] or bool(m.play) != bool(first.play):
                raise ValueError("from_maps: levels %r and %r differ in subtask order or `play`" % (first.name, m.name))
        K = len(lvs)
        if group_map is not None and envs_per_map is not None:
            raise ValueError("from_maps: pass group_map or envs_per_map, not both")
        if envs_per_map is not None:
            counts = [int(c) for c in envs_per_map]
            if len(counts) != K or any(c < 0 for c in counts):
                raise ValueError("from_maps: envs_per_map needs one non-negative count per level")
            if any(c % 64 for c in counts[:-1]):
                raise ValueError("from_maps: envs_per_map counts must be multiples of 64 (envs are assigned in groups "
                                 "of 64; only the last group of the batch may be partial): got %s" % counts)
            if num_envs is not None and int(num_envs) != sum(counts):
                raise ValueError("from_maps: num_envs disagrees with envs_per_map")
            num_envs = sum(counts)
            gm = np.concatenate([np.full((c + 63) // 64, m, np.int32) for m, c in enumerate(counts)])
        else:
            if num_envs is None:
                raise ValueError("from_maps: pass num_envs (with group_map, or alone) or envs_per_map")
            num_envs = int(num_envs)
            groups = (num_envs + 63) // 64
            if group_map is None:
                gm = (np.arange(groups) % K).astype(np.int32)
            else:
                gm = np.asarray(group_map)
                if gm.ndim != 1 or gm.size != groups or gm.dtype.kind not in "iu":
                    raise ValueError("from_maps: group_map must hold one map index per group of 64 envs: %d for %d "
                                     "envs (got shape %s)" % (groups, num_envs, gm.shape))
                if gm.size and (gm.min() < 0 or gm.max() >= K):
                    raise ValueError("from_maps: group_map values must lie in 0..%d (got %d..%d)"
                                     % (K - 1, gm.min(), gm.max()))
                gm = gm.astype(np.int32)
        if num_envs < 1:
            raise ValueError("from_maps: no envs")
        full = {"BLIND": False, "CAN_MOVE": True}
        players = [dict(full, **(kw.get(c) or {})) for c in ("ego_config", "partner_config")]
        std = (kw.get("communication_on", True) and not kw.get("ego_led", False) and kw.get("ego_agent_idx", 0) == 0
               and not first.play and all(c["CAN_MOVE"] and not c["BLIND"] for c in players))
        if not std:
            raise ValueError("from_maps: map sets run the wrapper's standard configuration (communication on, not "
                             "ego-led, both CAN_MOVE, ego_agent_idx 0, nobody BLIND, play off)")
        return cls(first, num_agents=2, num_envs=num_envs, _maps=(lvs, np.ascontiguousarray(gm)), **kw)

    def map_of(self, i):
        """Name of the level env i lives on."""
        if not 0 <= int(i) < self.n:
            raise IndexError("env index %d outside 0..%d" % (i, self.n - 1))
        return (self.levels[int(self.group_map_host[int(i) // 64])] if self.levels else self.level).name

    def level_of(self, i):
        """The ``CompiledLevel`` env i lives on."""
        return self.levels[int(self.group_map_host[int(i) // 64])] if self.levels else self.level

    def _single_level_only(self, what):
        if self.levels:
            raise ValueError("%s is not available for a map set (BatchedOvercooked.from_maps)" % what)

    def get_state(self):
        """Everything that carries the batch from one step to the next -- the arena (state, comm, done,
        outputs, episode statistics), the placement stream and the metrics -- as device copies."""
        cl = lambda t: None if t is None else t.clone()
        return {"arena": self._arena.clone(), "rng": cl(self.rng), "metrics": cl(self.metrics)}

    def set_state(self, st):
        """Put a ``get_state()`` of this batch (or of one of the same shape) back."""
        self._arena.copy_(st["arena"])
        for name in ("rng", "metrics"):
            if getattr(self, name) is not None:
                getattr(self, name).copy_(st[name])

    @property
    def launch_waves_per_64(self):
        """Waves per 64 envs the PLAIN fused step is launched with (1, 2 or 4 = split launches)."""
        return self.launch_waves(general=False)

    @property
    def standard_wrapper_config(self):
        """The wrapper configuration of the reference's own run files (communication on, not ego-led,
        both players CAN_MOVE, ego = sim agent 0, nobody BLIND, play off): what the plain step and
        the options-on-the-standard-configuration variant of the fused kernel fold at compile time
        (csrc/oc_kernels.hip: MultiVariant, xo = 0 / 1); anything else runs the general variant."""
        c = self._wrap_cfg
        return bool(c.communication_on and not c.ego_led and c.can_move_mask == 3 and c.ego_agent_idx == 0
                    and c.obs.blind_mask == 0 and not self.level.play)

    def launch_waves(self, general=False):
        """Waves per 64 envs the library launches for this batch (include/oc_hip.h:
        oc_multi_step_waves): the plain step, or -- ``general`` -- the general variant (pairs /
        in-kernel partner / episode statistics / policies / a non-standard wrapper configuration:
        what ``OvercookedVecEnv`` launches), which splits four ways or not at all."""
        return int(getattr(self._L, self._fn["multi_step_waves"])(self.n, self.waves_per_64, 1 if general else 0))

    def launch_lanes(self, general=False):
        """Lanes per env of that launch (include/oc_hip.h: oc_multi_step_lanes): 1, or 2 where
        the library lane-splits the plain step's four-way split at a small batch."""
        if self.levels:
            return 1
        return int(self._L.oc_multi_step_lanes(self.n, self.waves_per_64, 1 if general else 0))

    # -- helpers ---------------------------------------------------------------
    def _on_device(self):
        """Kernels must be launched with this env's device current."""
        return _lib.on_device(self._dev_index)

    def _call(self, name, *args, stream=True):
        """Entry point `name` of this env's library on its device and torch's current stream (not
        for the per-step paths below, whose cost is counted in single ctypes calls)."""
        _lib.call(self._L, name, self._dev_index, *args, stream=stream)

    @staticmethod
    def _p(t: Optional[torch.Tensor]):
        return ctypes.c_void_p(0 if t is None else t.data_ptr())

    def _check_tensor(self, t, shape, dtype, name):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor" % name)
        if t.device != self.state.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s on %s (got %s %s %s)"
                             % (name, dtype, tuple(shape), self.state.device, t.dtype,
                                tuple(t.shape), t.device))

    # -- API -------------------------------------------------------------------
    def reset(self, mask: Optional[torch.Tensor] = None):
        """Reset all envs, or those with mask[n] != 0 (int32 [n])."""
        if mask is not None:
            self._check_tensor(mask, (self.n,), torch.int32, "mask")
        self._call(self._fn["reset"], *self._lead, self._p(self.state), self._p(mask), self._p(self.placement),
                   self._p(self.rng), self.n)

    def set_placement(self, placement: torch.Tensor):
        """placement_mode='host': the start cells (int32 [M][n], x | y<<4, world order) every
        env uses at its next reset / auto-reset."""
        if self.placement is None:
            raise ValueError("this env was not created with placement_mode='host' on a random-* level")
        self._check_tensor(placement, (self.M, self.n), torch.int32, "placement")
        self.placement.copy_(placement)

    def step(self, actions: torch.Tensor, auto_reset: Optional[bool] = None):
        """Base-env step.  actions: int32 [A][n] action codes 0..4 (4 = stay).
        Returns (reward int32[n], done int32[n], shaping f64[2][n]) -- views of
        pre-allocated tensors, overwritten by the next call."""
        self._single_level_only("the base step")
        self._check_tensor(actions, (self.A, self.n), torch.int32, "actions")
        ar = self.auto_reset if auto_reset is None else auto_reset
        self._call("oc_step", self._h, self._p(self.state), self._p(actions), self._p(self.reward),
                   self._p(self.done), self._p(self.shaping), int(ar), self._p(self.metrics),
                   self._p(self.placement), self._p(self.rng), self.n)
        return self.reward, self.done, self.shaping

    def observe(self):
        """Both viewers' observations of the current state.  Returns (obs int32 [2][F][n],
        timestep f64 [n])."""
        self._call(self._fn["obs"], *self._lead, self._p(self.state), self._p(self.comm), ctypes.byref(self._obs_cfg),
                   self._p(self.obs), self._p(self.timestep), self.n)
        return self.obs, self.timestep

    def multi_step(self, actions: Optional[torch.Tensor] = None, auto_reset: Optional[bool] = None,
                   ego_pairs: Optional[torch.Tensor] = None, alt_pairs: Optional[torch.Tensor] = None,
                   alt_rng: Optional[torch.Tensor] = None, alt_played: Optional[torch.Tensor] = None,
                   policy=None):
        """gym_comm wrapper step in one launch.  actions: int32 [4][n] = ego move (0..3),
        ego comm, alt move, alt comm.  Per player the (move, comm) may instead come as an
        int32 or int64 [n][2] tensor of pairs (`ego_pairs` / `alt_pairs`: a policy's [n, 2] output as it
        lies), and the partner may be drawn by the kernel itself, uniformly, from a per-env
        PCG32 stream (`alt_rng`, int32/uint32 [n]; `alt_played` int32 [2][n] receives the draw)
        -- include/oc_hip.h, oc_step_opts.  `policy`: a pair of device-address tuples
        (w1, w2, b2, rng or None) -- the two players' packed MLPs (include/oc_policy.h): the kernel
        evaluates them behind the step and overwrites `ego_pairs` / `alt_pairs` (int32) with the
        NEXT step's actions: the closed loop in one launch.
        Returns (obs, timestep, shaped_reward f64[n], done)."""
        n = self.n
        if actions is not None:
            self._check_tensor(actions, (4, n), torch.int32, "actions")
        elif ego_pairs is None or (alt_pairs is None and alt_rng is None):
            raise ValueError("multi_step needs `actions`, or `ego_pairs` and one of `alt_pairs` / `alt_rng`")
        pdt = None
        for name, t in (("ego_pairs", ego_pairs), ("alt_pairs", alt_pairs)):
            if t is not None:
                if t.dtype not in (torch.int32, torch.int64) or (pdt is not None and t.dtype != pdt):
                    raise ValueError("ego_pairs / alt_pairs must be int32 or int64, both the same")
                pdt = t.dtype
                self._check_tensor(t, (n, 2), pdt, name)
        if alt_rng is not None:
            self._check_tensor(alt_rng, (n,), torch.int32, "alt_rng")
        if alt_played is not None:
            self._check_tensor(alt_played, (2, n), torch.int32, "alt_played")
        ptr = lambda t: None if t is None else t.data_ptr()
        if policy is not None:
            self._single_level_only("policy= (the fused policies)")
            if ego_pairs is None or alt_pairs is None or pdt is not torch.int32 or alt_rng is not None:
                raise ValueError("policy= needs int32 ego_pairs and alt_pairs (it overwrites them) and no alt_rng")
            if self._policy_arr is None:
                self._policy_arr = (_lib.StepPolicy * 2)()
            for k, (w1, w2, b2, rng) in enumerate(policy):
                self._policy_arr[k] = _lib.StepPolicy(w1, w2, b2, rng)
        self.multi_step_raw(ptr(actions) or 0, ptr(ego_pairs), ptr(alt_pairs), ptr(alt_rng), ptr(alt_played),
                            int(self.auto_reset if auto_reset is None else auto_reset), pdt is torch.int64,
                            policy=self._policy_arr if policy is not None else None)
        return self.obs, self.timestep, self.shaped_reward, self.done

    def multi_step_raw(self, actions_ptr, ego_pairs_ptr, alt_pairs_ptr, alt_rng_ptr, alt_played_ptr, auto_reset,
                       pairs_int64=False, policy=None):
        """multi_step on raw device addresses (int, None = absent), nothing checked: the per-call
        cost is one ctypes call.  For callers that validated their tensors once (vec_env)."""
        a = self._ms_args
        if a is None:       # every pointer but the action sources is fixed for the life of the env
            dp = lambda t: 0 if t is None else t.data_ptr()
            self._ms_opts = _lib.StepOpts(dp(self.ep_return) or None, dp(self.ep_length) or None,
                                          None, None, None, None, 0, self.waves_per_64)
            a = self._ms_args = [*self._lead, dp(self.state), dp(self.comm), 0, ctypes.byref(self._wrap_cfg),
                                 dp(self.obs), dp(self.timestep), dp(self.shaped_reward), dp(self.done),
                                 dp(self.reward), 0, dp(self.metrics), dp(self.placement), dp(self.rng),
                                 ctypes.byref(self._ms_opts), self.n, 0]
            self._ms_fn = getattr(self._L, self._fn["multi_step"])
        o = self._ms_opts
        k = len(self._lead) - 1     # (a map set's calls carry group_map behind the handle)
        o.ego_pairs, o.alt_pairs, o.alt_rng, o.alt_played = ego_pairs_ptr, alt_pairs_ptr, alt_rng_ptr, alt_played_ptr
        o.pairs_int64 = 1 if pairs_int64 else 0
        o.policy = policy if policy is not None else None    # (_lib.StepPolicy * 2) or NULL
        a[3 + k] = actions_ptr
        a[10 + k] = auto_reset
        a[16 + k] = self._raw_stream()
        if torch.cuda.current_device() == self._dev_index:
            rc = self._ms_fn(*a)
        else:
            with torch.cuda.device(self.device):
                rc = self._ms_fn(*a)
        if rc:
            _lib.check(rc, self._fn["multi_step"], self._L)

    def prepare_multi_step(self, actions_ptr, alt_rng_ptr=None, alt_played_ptr=None, alt_pairs_ptr=None,
                           auto_reset=True):
        """A PREPARED fused step (include/oc_hip.h: oc_multi_step_prepare): every argument but the ego's
        pair tensor fixed once; returns a ``PreparedStep``: ``launch(ego_pairs_ptr_or_None, pairs_int64)``, whose
        per-call cost is a 4-argument foreign call (the 17-argument one costs a Python caller ~2 us more), and
        ``close()``.  The env's tensors must not be rebound while a prepared step is alive."""
        dp = lambda t: 0 if t is None else t.data_ptr()
        if self.levels:     # (no prepared form for map sets: the same launch through multi_step_raw)
            def launch_set(ego_pairs_ptr=None, pairs_int64=False):
                self.multi_step_raw(actions_ptr or 0, ego_pairs_ptr, alt_pairs_ptr, alt_rng_ptr, alt_played_ptr,
                                    int(auto_reset), pairs_int64)
            return PreparedStep(launch_set)
        opts = _lib.StepOpts(dp(self.ep_return) or None, dp(self.ep_length) or None, None, alt_pairs_ptr,
                             alt_rng_ptr, alt_played_ptr, 0, self.waves_per_64)
        h = ctypes.c_void_p()
        self._call("oc_multi_step_prepare", self._h, dp(self.state), dp(self.comm), actions_ptr or 0,
                   ctypes.byref(self._wrap_cfg), dp(self.obs), dp(self.timestep), dp(self.shaped_reward),
                   dp(self.done), dp(self.reward), int(auto_reset), dp(self.metrics), dp(self.placement),
                   dp(self.rng), ctypes.byref(opts), self.n, ctypes.byref(h), stream=False)
        L, dev, call = self._L, self._dev_index, h
        raw_stream = torch._C._cuda_getCurrentRawStream

        def launch(ego_pairs_ptr=None, pairs_int64=False):
            if torch.cuda.current_device() == dev:
                rc = L.oc_call_launch(call, ego_pairs_ptr, 1 if pairs_int64 else 0, raw_stream(dev))
            else:
                with torch.cuda.device(dev):
                    rc = L.oc_call_launch(call, ego_pairs_ptr, 1 if pairs_int64 else 0, raw_stream(dev))
            if rc:
                _lib.check(rc, "oc_call_launch", L)
        return PreparedStep(launch, L, h, self._prepared)

    def observe_image(self, radius: Optional[int] = None, packed: bool = False):
        """Image-style fog-of-war observation of both viewers
        (get_partial_observability_FOW, overcooked_env.py:161-202).  Returns
        (maps int8 [2][7][W][H][n], holding int8 [2][n]).  The kernel writes four consecutive
        cells of a plane of an env per dword ([2][7*ceil(WH/4)][n] int32, include/oc_hip.h); the
        [2][7][W][H][n] result is one re-layout copy of that -- `packed=True` returns the
        kernel's tensor itself."""
        self._single_level_only("observe_image")
        lv = self.level
        if getattr(self, "_image", None) is None:
            self._image_words = self._L.oc_image_words(self._h)
            self._image = torch.zeros((2, self._image_words, self.n), dtype=torch.int32, device=self.device)
            self._holding = torch.zeros((2, self.n), dtype=torch.int8, device=self.device)
        r = self._obs_cfg.fow_radius if radius is None else int(radius)
        self._call("oc_obs_image", self._h, self._p(self.state), r, self._p(self._image), self._p(self._holding),
                   self.n)
        if packed:
            return self._image, self._holding
        cells = lv.width * lv.height
        q = self._image_words // 7
        img = self._image.view(torch.int8).view(2, 7, q, self.n, 4).permute(0, 1, 2, 4, 3).reshape(2, 7, 4 * q, self.n)
        return img[:, :, :cells].reshape(2, 7, lv.width, lv.height, self.n), self._holding

    def completed_subtasks(self):
        """completed_subtasks of every env as int32 [S][n] (from the packed state)."""
        word = self.state[self.A + self.M]
        if getattr(self, "_slot_t", None) is None:
            self._slot_t = torch.tensor(self.subtask_slot, device=self.device, dtype=torch.int32).view(-1, 1)
        return (word.view(1, -1) >> self._slot_t) & 1

    def obs_dict(self, viewer: int):
        """The 11 observation keys of get_observation2 as tensor views: key -> [k][n]
        (``.T`` gives the [n][k] batch a policy takes); 'timestep' is f64 [1][n]."""
        d = {"timestep": self.timestep.unsqueeze(0)}
        for k, (a, b) in self._layout.items():
            d[k] = self.obs[viewer, a:b]
        return d

    def snapshot(self):
        """Named fields of every env's state (host numpy), see state.unpack_state."""
        return unpack_state(self.state.cpu().numpy(), self.A, self.M, self.S, **self.unpack_kw())

    def unpack_kw(self):
        """Extra arguments state.unpack_state needs for this level: the bit of every subtask in
        the state's subtask words and, in dup mode, where its goal count lives."""
        kw = {"slot": self.subtask_slot}
        if self._dup:
            kw.update(goal_index=self._goal_index,
                      deliver=[s.kind == compiler.KIND_DELIVER for s in self.level.subtasks])
        return kw

    def fetch(self):
        """ONE device->host copy of everything a step produced: returns {name: numpy view}
        for state, reward, done, shaping, comm, obs, timestep, shaped_reward (host copies
        with the device tensors' shapes and dtypes).  Synchronises with the stream."""
        # through a pinned staging buffer (an asynchronous copy + one stream sync: about half the
        # latency of a pageable .cpu() for the single-env adapter's 1 KB arena), then a host copy
        # so that the caller owns what it gets
        if self._arena_pinned is None:
            self._arena_pinned = torch.empty(self._arena.numel(), dtype=torch.uint8, pin_memory=True)
        self._arena_pinned.copy_(self._arena, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        host = self._arena_pinned.numpy().copy()
        if self._fetch_plan is None:
            self._fetch_plan = [(name, o, o + nb, np.dtype(str(dt).replace("torch.", "")), shape)
                                for name, (o, nb, shape, dt) in self._arena_layout.items()]
        return {name: host[lo:hi].view(ndt).reshape(shape) for name, lo, hi, ndt, shape in self._fetch_plan}

    def metrics_vector(self):
        """int64[8] totals (sum over the per-wave slots), on the device; None when the env was
        built with track_metrics=False."""
        if self.metrics is None:
            return None
        return self.metrics.sum(dim=0)

    def read_metrics(self):
        if self.metrics is None:
            return None
        name = lambda m: {"env_steps": m[0], "episodes": m[1], "successes": m[2], "reward_sum": m[3],
                          "completed_subtasks_sum": m[4], "errors": m[5]}
        if not self.levels:
            return name(self.metrics_vector().cpu().tolist())
        # a map set: one slot per group of 64 envs, so a map's counters are the sum of its groups' slots
        slots = self.metrics.cpu().numpy()[:self.group_map_host.size]
        out = name(slots.sum(axis=0).tolist())
        out["per_map"] = [dict(name(slots[self.group_map_host == m].sum(axis=0).tolist()), level=lv.name)
                          for m, lv in enumerate(self.levels)]
        return out
