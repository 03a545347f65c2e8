"""Vectorised trainer boundary: N Overcooked envs behind the
Stable-Baselines3 ``VecEnv`` API, ego-perspective, with the partner policy evaluated on
the whole batch.

The reference trains on ONE env: ``RecurrentPPO`` wraps ``OvercookedMultiEnv`` in
``Monitor + DummyVecEnv(1)`` and pantheonrl asks the partner agent for one action per
step (pantheonrl/common/multiagentenv.py:149-215, trainer.py:87-121).  Here the same
ego/partner protocol runs on tensors:

    obs_ego = venv.reset()
    obs_ego, rewards, dones, infos = venv.step(ego_actions)      # ego_actions [n, 2] = (move, comm)

Call order of one step, as ``MultiAgentEnv.step`` (multiagentenv.py:149-215):
``partner.act_into(obs_partner)`` on the observations the partner saw after the previous step
(``_get_actions``: ``agent.get_action(ob)``, SimultaneousEnv semantics :395-404); the fused
``oc_multi_step`` kernel once (``n_step``); ``partner.update(rewards, dones)`` if the partner
has that method (``_update_players`` -> ``OnPolicyAgent.update``, agents.py:168-185).  Finished
envs are auto-reset inside the kernel, so -- as with any SB3 VecEnv -- the observation returned
for a done env is the first observation of its next episode and ``rewards``/``dones`` belong to
the finished step.  ``infos[i]["terminal_observation"]`` is only filled with
``terminal_obs=True`` (three launches per step instead of one).  Episode return / length
(what SB3's ``Monitor`` adds: ``infos[i]["episode"]``) are kept by the kernel itself.

Partners
  ``RandomPartner``        uniform random, drawn inside the step kernel (no launch of its own);
  ``TorchPolicyPartner``   any ``torch.nn.Module`` mapping the observation dict to (move logits,
                           comm logits) -- the batched stand-in for pantheonrl's
                           ``OnPolicyAgent.get_action`` / ``update`` (agents.py:112-194);
  ``RecurrentPolicyPartner``  a STATEFUL torch policy (per-env recurrent state, ``episode_start``
                           masks, log-probs / values, a graph-capturable ``RolloutSink``) -- what
                           the reference seats there: ``OnPolicyAgent(RecurrentPPO(...))``;
  ``FusedMLPPartner``      an ``MLPPolicy`` (64 tanh units) as ONE launch of the hand-written MFMA
                           policy kernel (include/oc_policy.h), ego and partner in the same launch;
  ``FusedActorCriticPartner``  an ``MLPActorCritic`` in the seat of a player that learns: action,
                           log-probability and value from one launch, recorded into a ``RolloutSink``;
                           ``PPOLearner`` (learner.py) is its update: loss, backward, clip, Adam and
                           the repack of the seat's weights in three launches per minibatch;
  ``FusedRecurrentPartner``  an ``LSTMActorCritic`` in the seat of a recurrent player, one launch per step;
                           ``RecurrentPPOLearner`` (learner.py) is its update over whole recorded sequences:
                           forward, backpropagation through time, clip, Adam and the repack in six launches,
                           or over windows of the rollout from the states the seat recorded every W steps
                           (``RolloutSink(state_window=W)``, ``train_windows``): one gather launch more;
  any callable ``partner(obs_dict) -> [n, 2]`` still works (slow path).
How a seated player yields its actions -- pairs consumed as they lie, ``act_into`` on the action
rows, a callable -- is decided in one place, ``seat_actions``, for the partner's seat and the ego's.

``ClosedLoop`` (``venv.closed_loop(ego)``) captures ego policy -> partner policy -> fused step
(+ in-kernel episode statistics) in one hipGraph, so a rollout costs one graph replay per step
(or per k steps) instead of a dozen host-side launches.  A loop keeps the partner it was built
with; assigning ``venv.partner`` retires the env's loops and closes its prepared step.

Subclasses ``stable_baselines3.common.vec_env.VecEnv`` when SB3 is importable; otherwise a
structural stand-in with the same methods.  ``step_tensors`` is the zero-copy variant for
policies that live on the GPU.  The numpy API is ``hostio.py``'s: a transport, built on the first
numpy call, packs a step's arrays with one launch of ``oc_pack_host`` (include/oc_hostio.h) and one
PCIe copy (``HostCopy``) -- or, with ``host_io="mapped"`` (``HostMapped``), has the kernels read the
actions from host-mapped memory and write the packed step into it, and finishes the step by polling
an event (no copy, no blocking wait).  This class validates, assembles ``infos`` and calls it.
"""
import os
import weakref

import numpy as np
import torch

from .batched import BatchedOvercooked
from .hostio import MappedBuffer, SPACE_DTYPE, TRANSPORTS  # noqa: F401 (re-exported)
from .envs import OvercookedEnvironment, _arg, make_spaces
from .partners import (FusedActorCriticPartner, FusedMLPPartner, FusedRecurrentPartner,  # noqa: F401 (re-exported)
                       LSTMActorCritic, MLPActorCritic, MLPPolicy, RandomPartner, RecurrentPolicyPartner,
                       TorchPolicyPartner)
from .rollout import RolloutSink  # noqa: F401 (re-exported)
from .learner import PPOLearner, RecurrentPPOLearner  # noqa: F401 (re-exported)

try:                                                    # pragma: no cover - SB3 absent in CI image
    from stable_baselines3.common.vec_env import VecEnv as _VecEnvBase
except Exception:
    class _VecEnvBase:                                  # structural stand-in
        def __init__(self, num_envs, observation_space, action_space):
            self.num_envs = num_envs
            self.observation_space = observation_space
            self.action_space = action_space

        def step(self, actions):
            self.step_async(actions)
            return self.step_wait()


class ObsView(dict):
    """One viewer's observation: the 11 keys of get_observation2 as [n, k] tensor views, plus
    the storage they are views of -- ``rows`` ([F][n], the kernel's env-major rows; a policy
    that consumes them feature-major needs no gather, transpose or concat) and ``timestep``
    (f64 [n]).  The same objects every step; the next step overwrites their contents."""
    rows = None
    timestep = None


def seat_actions(player, obs, rows):
    """How a seated player produces its (move, comm): the ONE place that knows.  ``obs``: the viewer's
    ``ObsView``; ``rows``: int32 [2][n], that seat's move and comm rows of the kernel's action tensor.
    Returns int32 [n][2] pairs for the step kernel to consume as they lie, or None after writing
    ``rows``.  A ``FusedMLPPartner`` yields its pairs (one launch); anything with ``act_into(obs,
    move_row, comm_row)`` writes the rows; a bare callable ``player(obs) -> [n, 2]`` is taken as it
    lies when int32 and contiguous, and copied into the rows otherwise.  (The in-kernel partner and
    the joint launch of two fused policies are decided in front of this, where they apply.)"""
    if isinstance(player, FusedMLPPartner):
        return player.pairs_for(obs)
    act_into = getattr(player, "act_into", None)
    if act_into is not None:
        act_into(obs, rows[0], rows[1])
        return None
    pa = torch.as_tensor(player(obs), device=rows.device)
    if pa.dtype == torch.int32 and pa.is_contiguous():
        return pa
    rows.copy_(pa.T)
    return None


class ClosedLoop:
    """ego policy -> partner policy -> fused step, ``steps`` times, as ONE hipGraph.

    ``ego``: any player ``seat_actions`` takes (``TorchPolicyPartner``, ``RandomPartner``, a
    ``FusedMLPPartner``, anything with ``act_into``, a callable), or None -- then the caller writes
    the ego's (move, comm) into ``venv.ego_action_rows`` before every ``step()``.  ``enqueue()``
    issues the launches of one step eagerly (what gets captured; also usable inside a caller's own
    capture).

    The loop keeps the partner it was built -- and captured -- with (``self.partner``).  Replacing
    ``venv.partner`` RETIRES every live loop of that env: ``step()`` / ``enqueue()`` then raise, and
    ``reset_tensors()`` no longer looks at it; build a new loop.  Two live one-launch loops that
    share players on one env are not supported: each would rewind the shared streams at a reset."""
    retired = False
    _RETIRED = ("the env's partner was replaced after this loop was built (and captured): build a new loop "
                "with venv.closed_loop(...)")

    def __init__(self, venv, ego=None, graph=True, steps=1, one_launch=None):
        self.venv, self.ego, self.steps = venv, ego, int(steps)
        self.partner = venv.partner
        self.graph = None
        # ego and partner both FusedMLPPartner: let the step kernel evaluate them (one launch per
        # step instead of two) where the library can -- a specialised one, at most 4 comm channels --
        # and where it pays: in a split launch each of the four waves takes one (viewer, half)
        # pass (7.7 -> 6.7 us per step at 4 096 envs); a lone wave per 64 envs would run all four
        # passes back to back (9.6 -> 13.7 us at 32 768 envs), so larger batches keep two launches
        pt = self.partner
        # two fused policies of one shape share ONE launch of the policy kernel (or of the step kernel)
        self._joint = (isinstance(ego, FusedMLPPartner) and isinstance(pt, FusedMLPPartner) and pt.F == ego.F
                       and pt.C == ego.C)
        can = (self._joint and ego.C <= 4 and venv._b.kernel_flavour == "spec"
               and venv._b.standard_wrapper_config and not venv._b.levels)     # (a map set has no fused policies)
        if one_launch and not can:
            raise ValueError("one_launch needs two FusedMLPPartner of one shape, C <= 4, a specialised library, "
                             "the wrapper's standard configuration and a single level (no map set)")
        self.one_launch = (can and venv._b.launch_waves(general=True) == 4) if one_launch is None else bool(one_launch)
        # MultiAgentEnv._update_players (multiagentenv.py:186-195): every seated agent hears the step's
        # reward and done -- inside the captured graph when the player's update() is device work
        self._updates = [pl.update for pl in (ego, pt) if pl is not None and hasattr(pl, "update")]
        self._primed = False
        self.prime()
        venv._loops.add(self)       # reset_tensors() re-primes every live loop (weak references)
        if graph:
            for pl in (ego, pt):
                if pl is not None and not getattr(pl, "graph_safe", False):
                    raise ValueError("%r is not marked graph_safe (stateless, fixed-shape)" % (pl,))
            self.graph = venv._capture(self.enqueue, players=[ego], repeat=self.steps)

    def prime(self):
        """One-launch closed loop only: ``ego.pairs`` / ``partner.pairs`` hold the NEXT step's actions,
        computed by the previous step's launch from the observations it wrote.  After anything that
        rewrites the observations behind the loop's back -- ``reset_tensors()`` above all, which
        calls this for every live loop -- they must be recomputed from the CURRENT observations (one
        eager launch of the policy kernel, outside any graph), or the first step after the reset
        would play actions sampled for the pre-reset state.  Order for a loop built
        before the first reset: ``closed_loop(...)``, ``reset_tensors()`` (primes), ``step()``..."""
        if not self.one_launch:
            return
        v = self.venv
        if self._primed:
            # the pending pairs being replaced consumed one draw of each stream: take it back, so the
            # re-evaluation on the new observations uses the draw the two-launch form would use next
            self.ego.rewind_rng()
            self.partner.rewind_rng()
        o0, o1 = v._obs_tensors(0), v._obs_tensors(1)
        FusedMLPPartner.launch([self.ego, self.partner], [o0.rows, o1.rows], o0.timestep)
        self._primed = True

    def enqueue(self):
        if self.retired:
            raise RuntimeError(self._RETIRED)
        v = self.venv
        ego, pt = self.ego, self.partner
        if self._joint:
            o0, o1 = v._obs_tensors(0), v._obs_tensors(1)
            if self.one_launch:
                # the step kernel evaluates both policies itself, behind the step, on the
                # observations it has just written, and leaves the NEXT step's pairs in
                # ego.pairs / pt.pairs (oc_step_opts.policy): ONE launch per step.  (The pairs
                # of the very first step came from one launch of the policy kernel: __init__.)
                n = v.num_envs
                v._b.multi_step(v._act, ego_pairs=ego.pairs, alt_pairs=pt.pairs,
                                policy=(ego.step_policy(n), pt.step_policy(n)))
            else:
                # both policies in ONE launch, their pairs consumed by the step as they lie
                FusedMLPPartner.launch([ego, pt], [o0.rows, o1.rows], o0.timestep)
                v._b.multi_step(v._act, ego_pairs=ego.pairs, alt_pairs=pt.pairs)
        else:       # (ego None: the caller wrote the ego's rows)
            v._partner_and_step(None if ego is None else seat_actions(ego, v._obs_tensors(0), v._seat_rows[0]))
        for update in self._updates:
            update(v._b.shaped_reward, v._b.done)
        v._version += 1

    def step(self):
        """Returns (ego obs, shaped reward f64 [n], done int32 [n]) -- views of the tensors the
        next step overwrites."""
        v = self.venv
        if self.retired:
            raise RuntimeError(self._RETIRED)
        if self.graph is not None:
            self.graph.replay()
            v._version += self.steps
        else:
            for _ in range(self.steps):
                self.enqueue()
        return v._obs_tensors(0), v._b.shaped_reward, v._b.done


class _MapOf:
    """A map set's batch as the per-env view sees it: ``level`` is the env's own map, the rest the batch's."""

    def __init__(self, batch, level):
        self._batch, self.level = batch, level

    def __getattr__(self, name):
        return getattr(self._batch, name)


class OvercookedVecEnv(_VecEnvBase):
    def __init__(self, arglist, num_envs, partner=None, device="cuda", terminal_obs=False,
                 ego_agent_idx=0, subtask_order=None, level_dir=None, seed=0,
                 track_episode_stats=True, use_graph=False, reuse_host_buffers=False, levels=None,
                 group_map=None, envs_per_map=None, host_io="copy", **batched_kw):
        """``levels``: a list of level names / compiled levels of ONE structure -- the envs then live on
        different maps (``BatchedOvercooked.from_maps``; ``group_map`` / ``envs_per_map`` assign them in
        groups of 64, round-robin by default) and ``arglist.level`` is not looked at.

        ``host_io``: how the numpy API crosses PCIe.  ``"copy"``: staged copies in and out and a
        blocking wait.  ``"mapped"``: the step kernel reads the actions from host-mapped memory,
        ``oc_pack_host_tiled`` writes the packed step into one of two alternating host-mapped
        buffers, ``step_async`` starts that work and ``step_wait`` polls for its end."""
        if host_io not in tuple(TRANSPORTS):
            raise ValueError("host_io must be \"copy\" or \"mapped\", not %r" % (host_io,))
        if _arg(arglist, "num_agents") != 2:
            raise ValueError("the gym_comm wrapper drives exactly 2 agents")
        self.arglist = arglist
        self.terminal_obs = bool(terminal_obs)
        self.track_episode_stats = bool(track_episode_stats)
        if levels is None and (group_map is not None or envs_per_map is not None):
            raise ValueError("group_map / envs_per_map belong to levels=[...]")
        make = BatchedOvercooked if levels is None else \
            (lambda level, **kw: BatchedOvercooked.from_maps(levels, group_map=group_map, envs_per_map=envs_per_map, **kw))
        self._b = make(
            _arg(arglist, "level"), num_agents=2, num_envs=num_envs,
            max_num_timesteps=_arg(arglist, "max_num_timesteps", 100),
            max_num_subtasks=_arg(arglist, "max_num_subtasks", 14),
            ego_config=dict(_arg(arglist, "ego_config", {}) or {}),
            partner_config=dict(_arg(arglist, "partner_config", {}) or {}),
            num_communication=_arg(arglist, "num_communication", 10),
            communication_on=_arg(arglist, "communication_on", False),
            ego_led=_arg(arglist, "ego_led", False), fow_radius=_arg(arglist, "fow_radius", 2),
            ego_agent_idx=ego_agent_idx, device=device, subtask_order=subtask_order,
            level_dir=level_dir, auto_reset=True, seed=seed,
            episode_stats=self.track_episode_stats, play=bool(_arg(arglist, "play", False)), **batched_kw)
        lv = self._b.level
        obs_space, act_space = make_spaces(lv.width, lv.height, lv.num_subtasks, self._b.C)
        super().__init__(num_envs, obs_space, act_space)
        self._fast = self._graph = None
        self._loops = weakref.WeakSet()                  # live ClosedLoop objects (re-primed by reset_tensors)
        self.partner = partner if partner is not None else RandomPartner(self._b.C, seed, self._b.device)
        self._act = torch.zeros((4, num_envs), dtype=torch.int32, device=self._b.device)
        self._seat_rows = (self._act[0:2], self._act[2:4])     # (move, comm) rows of the ego and of the partner
        # the kernel overwrites the same observation rows every step, so the 11-key views of
        # both viewers are built once (22 slice + transpose objects cost ~60 us per step otherwise)
        self._views = [None, None]
        self._infos = [{} for _ in range(num_envs)]      # reused; only finished envs are touched
        self._dirty = []
        self._last_terminal = None
        self._version = 0                                # bumped by every step / reset
        self._env_views = {}                             # env index -> (OvercookedEnvironment view, version)
        self._env_attrs = {}                             # (env index, name) -> value set by set_attr(indices=...)
        self._use_graph = bool(use_graph) and not self.terminal_obs
        self._ego_pairs = None
        # the numpy API's transport (hostio.py), built on first use: tensor-only users allocate no pinned
        # or mapped memory.  reuse_host_buffers: False = every step returns fresh arrays; True = the arrays
        # are views of two alternating buffers, valid until the step after next
        self._io, self._io_args = None, (TRANSPORTS[host_io], bool(reuse_host_buffers))

    @property
    def partner(self):
        return self._partner

    @partner.setter
    def partner(self, pt):
        """A new partner invalidates what was prepared or captured with the old one: the prepared
        single-launch step is closed, the captured step dropped, every live ``ClosedLoop`` retired."""
        self._partner = pt
        if self._fast:
            self._fast["prepared"].close()
        self._fast = self._graph = None
        for lp in list(self._loops):
            lp.retired = True
        self._loops.clear()

    # the running episode statistics live in the batch (kept by the kernel)
    @property
    def episode_returns(self):
        return self._b.ep_return

    @property
    def episode_lengths(self):
        return self._b.ep_length

    @property
    def ego_action_rows(self):
        """int32 [2][n]: the ego's (move, comm) rows of the kernel's action tensor."""
        return self._act[0:2]

    # -- tensors ---------------------------------------------------------------------
    def _obs_tensors(self, viewer):
        """The 11 keys as [n, k] device tensors (views of the kernel's [k][n] rows; the same
        tensor objects every step -- the next step overwrites their contents)."""
        if self._views[viewer] is None:
            d = self._b.obs_dict(viewer)
            v = ObsView((k, t.T) for k, t in d.items())
            v.rows, v.timestep = self._b.obs[viewer], self._b.timestep
            self._views[viewer] = v
        return self._views[viewer]

    def reset_tensors(self):
        b = self._b
        b.reset()
        b.done.zero_()
        if self.track_episode_stats:
            b.ep_return.zero_()
            b.ep_length.zero_()
        b.observe()
        self._version += 1
        # players with per-episode state start over (a recurrent partner's states and episode_start),
        # and every live one-launch closed loop recomputes its pending actions from the new observations
        seen = set()
        for pl in [self.partner] + [lp.ego for lp in self._loops]:
            if pl is not None and id(pl) not in seen and hasattr(pl, "reset"):
                seen.add(id(pl))
                pl.reset()
        for lp in self._loops:
            lp.prime()
        return self._obs_tensors(0)

    def closed_loop(self, ego=None, graph=True, steps=1, one_launch=None):
        """ego policy -> partner policy -> fused step as one hipGraph (see ``ClosedLoop``)."""
        return ClosedLoop(self, ego, graph=graph, steps=steps, one_launch=one_launch)

    def _fast_plan(self):
        """Addresses for the single-launch path of step_tensors, or False when it does not apply
        (a partner with launches or an update() of its own, terminal_obs, a captured graph)."""
        pt = self.partner
        if self._use_graph or self.terminal_obs or not getattr(pt, "in_kernel", False) or hasattr(pt, "update"):
            return False
        rng = pt.rng_state(self.num_envs).data_ptr()
        prepared = self._b.prepare_multi_step(self._act.data_ptr(), alt_rng_ptr=rng,
                                              alt_played_ptr=self._act[2:4].data_ptr(), auto_reset=True)
        return {"obs": self._obs_tensors(0), "pair_shape": torch.Size((self.num_envs, 2)), "dev": self._b._dev_index,
                # the prepared call (include/oc_hip.h: oc_multi_step_prepare): everything but the ego's pairs fixed
                "prepared": prepared, "launch": prepared.launch}

    def _capture(self, fn, players=(), repeat=1):
        """`repeat` calls of fn() as one hipGraph.  One eager warm-up call first (module loads,
        rocBLAS workspaces) that must not count: the env's tensors, the action rows, the metrics
        and every random stream (the env's, the players', torch's) are put back afterwards."""
        b = self._b
        if not getattr(self.partner, "graph_safe", False):
            raise ValueError("%r is not marked graph_safe (stateless, fixed-shape)" % (self.partner,))
        players = [pl for pl in list(players) + [self.partner] if pl is not None]
        keep, act = b._arena.clone(), self._act.clone()
        rng = None if b.rng is None else b.rng.clone()
        met = None if b.metrics is None else b.metrics.clone()
        torch_rng = torch.cuda.get_rng_state(b.device)
        saved = [pl.get_state(self.num_envs) if hasattr(pl, "get_state") else None for pl in players]
        ver = self._version
        fn()
        torch.cuda.current_stream(b.device).synchronize()
        b._arena.copy_(keep)
        self._act.copy_(act)
        if rng is not None:
            b.rng.copy_(rng)
        if met is not None:
            b.metrics.copy_(met)
        torch.cuda.set_rng_state(torch_rng, b.device)
        for pl, st in zip(players, saved):
            if hasattr(pl, "set_state"):
                pl.set_state(st)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(repeat):
                fn()
        self._version = ver
        return graph

    def _partner_and_step(self, ego_pairs, auto_reset=None):
        """The partner's move and the fused step.  ego_pairs: the ego's int32 [n][2] (move, comm)
        pairs, or None = rows 0, 1 of ``self._act``.  Launches: none for an in-kernel partner
        (``RandomPartner``), the partner's own otherwise; then ONE for the step."""
        b, pt = self._b, self.partner
        if getattr(pt, "in_kernel", False):
            b.multi_step(self._act, auto_reset=auto_reset, ego_pairs=ego_pairs,
                         alt_rng=pt.rng_state(self.num_envs), alt_played=self._act[2:4])
            return
        # rows of the action tensor: ego move, ego comm, alt move, alt comm
        alt_pairs = seat_actions(pt, self._obs_tensors(1), self._seat_rows[1])
        b.multi_step(self._act, auto_reset=auto_reset, ego_pairs=ego_pairs, alt_pairs=alt_pairs)

    def _staged_pairs(self):
        """int32 [n][2] on the device: where ego actions that the kernel cannot take as they lie are
        staged (allocated on first use; the captured step's fixed input)."""
        if self._ego_pairs is None:
            self._ego_pairs = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self._b.device)
        return self._ego_pairs

    def _single_launch(self):
        """``_fast_plan()``, made once per partner."""
        if self._fast is None:
            self._fast = self._fast_plan()
        return self._fast

    def _fast_step(self, f, ego_ptr, pairs_int64):
        """The single-launch step of ``_fast_plan()`` on the ego pairs at device address ``ego_ptr``
        (None: the ego's rows of ``self._act``), and the bookkeeping of a step."""
        f["launch"](ego_ptr, pairs_int64)
        self._version += 1
        self._last_terminal = None
        return f["obs"], self._b.shaped_reward, self._b.done

    def step_tensors(self, ego_actions=None):
        """ego_actions: int tensor [n, 2] on the device (None: already written into
        ``ego_action_rows``).  A contiguous int32 or int64 tensor is handed to the kernel as it
        lies (no copy, no extra launch).  Returns (ego obs dict of [n, k] tensors, shaped reward f64 [n],
        done int32 [n]) -- views that the next step overwrites."""
        b = self._b
        f = self._fast
        if f is None:
            f = self._fast = self._fast_plan()
        if f:   # one launch, no partner launch, nothing to capture: the per-call cost is one ctypes call
            ego_ptr = None
            if ego_actions is not None:
                ea = ego_actions
                if not (isinstance(ea, torch.Tensor) and (ea.dtype is torch.int32 or ea.dtype is torch.int64)
                        and ea.is_cuda and ea.is_contiguous() and ea.shape == f["pair_shape"]
                        and ea.get_device() == f["dev"]):
                    ea = self._staged_pairs()
                    ea.copy_(torch.as_tensor(ego_actions, device=b.device))
                ego_ptr = ea.data_ptr()
                i64 = ea.dtype is torch.int64
            return self._fast_step(f, ego_ptr, ego_ptr is not None and i64)
        ego_pairs = None
        if ego_actions is not None:
            ea = torch.as_tensor(ego_actions, device=b.device)
            if ea.dtype == torch.int32 and ea.is_contiguous() and not self._use_graph:
                ego_pairs = ea                 # (the slow path keeps to int32: alt_pairs may join it)
            else:                       # other dtypes / layouts, or the captured graph's fixed input
                ego_pairs = self._staged_pairs()
                ego_pairs.copy_(ea)
        term = None
        if self._use_graph:
            if ego_pairs is None:       # ego rows written by the caller: bring them into the graph's input
                self._staged_pairs().copy_(self._act[0:2].T)
            if self._graph is None:     # partner -> fused step (-> the partner's update), captured once
                def one_step():
                    self._partner_and_step(self._ego_pairs)
                    if hasattr(self.partner, "update"):
                        self.partner.update(b.shaped_reward, b.done)
                self._graph = self._capture(one_step)
            self._graph.replay()
            self._version += 1
            self._last_terminal = None
            return self._obs_tensors(0), b.shaped_reward, b.done
        else:
            if self.terminal_obs:
                self._partner_and_step(ego_pairs, auto_reset=False)
                term = {k: v.clone() for k, v in self._obs_tensors(0).items()}
                b.reset(b.done)                                   # mask = done flags
                b.observe()
            else:
                self._partner_and_step(ego_pairs)
            self._version += 1
        rew, done = b.shaped_reward, b.done
        self._last_terminal = term
        if hasattr(self.partner, "update"):
            self.partner.update(rew, done)
        return self._obs_tensors(0), rew, done

    # -- SB3 VecEnv API (numpy) --------------------------------------------------------
    @staticmethod
    def _to_numpy(obs):
        return {k: v.cpu().numpy().astype(SPACE_DTYPE[k]) for k, v in obs.items()}

    def _transport(self):
        """The numpy boundary's transport (hostio.py: ``HostCopy`` or ``HostMapped``), built on first use."""
        if self._io is None:
            cls, reuse = self._io_args
            self._io = cls(weakref.proxy(self), reuse)
        return self._io

    def reset(self):
        self.reset_tensors()
        return self._transport().observe()

    def step_async(self, actions):
        self._transport().start(actions)

    def step_wait(self):
        obs_np, rew_np, done_i32, stats = self._transport().finish()
        done_np = done_i32.astype(bool)
        infos = self._infos                       # the same list every step (as DummyVecEnv's buf_infos)
        for i in self._dirty:
            infos[i] = {}
        idx = np.nonzero(done_np)[0]
        self._dirty = idx.tolist()
        if len(idx):
            term = self._to_numpy(self._last_terminal) if self._last_terminal is not None else None
            if self.track_episode_stats:
                # after a step that returned done the kernel's rows hold the finished episode's
                # totals; they crossed PCIe with the observation (oc_pack_host)
                ret, ln = stats
            for i in idx:
                if self.track_episode_stats:
                    infos[i]["episode"] = {"r": float(ret[i]), "l": int(ln[i])}     # Monitor-style
                if term is not None:
                    infos[i]["terminal_observation"] = {k: v[i] for k, v in term.items()}
        return obs_np, rew_np, done_np, list(infos)   # shallow copy: holders keep their dicts

    def close(self):
        if self._io is not None:            # (a started step nobody waited for ends first)
            self._io.close()

    def seed(self, seed=None):
        return [seed] * self.num_envs

    # -- per-env access (VecEnv.get_attr / env_method) -------------------
    # ParallelEpisodeRecorder reads env.get_attr('t' | 'world' | 'sim_agents' | 'arglist', i)[0]
    # and keeps the world / sim_agents objects between steps (episode_recorder.py:48-85), so the
    # view of env i is ONE persistent object whose mirror is refreshed from the device -- a
    # column of A+M+2 state words -- when it is read after the batch has moved on.
    def _indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        idx = [int(i) for i in np.atleast_1d(indices)]
        for i in idx:
            if not 0 <= i < self.num_envs:
                raise IndexError("env index %d outside 0..%d" % (i, self.num_envs - 1))
        return idx

    def base_env(self, i):
        """The ``OvercookedEnvironment``-shaped view of env i (read-only; ``t``, ``world``,
        ``sim_agents``, ``completed_subtasks``, ``rep``, ``str()``, ``display()``,
        ``render_frame()``)."""
        i = self._indices([i])[0]
        ent = self._env_views.get(i)
        if ent is None:
            b = _MapOf(self._b, self._b.level_of(i)) if self._b.levels else self._b      # env i on its own map
            ent = [OvercookedEnvironment(self.arglist, _batch=b, _index=i, _view=True), -1]
            self._env_views[i] = ent
        if ent[1] != self._version:
            ent[0].mark_dirty()
            ent[1] = self._version
        return ent[0]

    _PER_ENV_ATTRS = ("base_env", "t", "world", "sim_agents", "completed_subtasks", "goal_objects_count",
                      "rep", "all_subtasks", "recipes")

    def get_attr(self, attr_name, indices=None):
        idx = self._indices(indices)
        if attr_name == "base_env":
            return [self.base_env(i) for i in idx]
        if attr_name in self._PER_ENV_ATTRS:
            return [getattr(self.base_env(i), attr_name) for i in idx]
        # an attribute set for some envs only (set_attr with indices) lives on those envs' views
        return [self._env_attrs[(i, attr_name)] if (i, attr_name) in self._env_attrs else getattr(self, attr_name)
                for i in idx]

    def set_attr(self, attr_name, value, indices=None):
        """SB3's ``VecEnv.set_attr``: the attribute of the envs in ``indices`` (None = all).  The
        device state of an env is not settable this way (the per-env views are read-only mirrors):
        state-derived names raise.  ``indices=None`` sets a batch-level attribute of the VecEnv;
        a subset is remembered per env and returned by ``get_attr`` for those envs."""
        if attr_name in self._PER_ENV_ATTRS:
            raise AttributeError("%r mirrors device state and is read-only" % attr_name)
        if indices is None:
            setattr(self, attr_name, value)
            for key in [k for k in self._env_attrs if k[1] == attr_name]:
                del self._env_attrs[key]
            return
        for i in self._indices(indices):
            self._env_attrs[(i, attr_name)] = value

    _PER_ENV_METHODS = ("render_frame", "render_rgb", "display", "get_agent_names", "__str__")

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        idx = self._indices(indices)
        if method_name in self._PER_ENV_METHODS:
            return [getattr(self.base_env(i), method_name)(*method_args, **method_kwargs) for i in idx]
        return [getattr(self, method_name)(*method_args, **method_kwargs)] * len(idx)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    def metrics(self):
        return self._b.read_metrics()


class BatchEpisodeRecorder:
    """``ParallelEpisodeRecorder`` (episode_recorder.py:48-85) for the batched env: wraps an
    ``OvercookedVecEnv``, counts episodes per env and, for the envs in ``indices`` whose episode
    number is a multiple of ``record_interval``, collects one frame per step --
    ``render_frame()`` of that env's view, i.e. the composition of the reference's pygame
    renderer from device state (the ASCII ``str(env)`` without sprites).  A finished episode's
    frames are handed to ``on_episode(env_index, episode, frames)`` (default: kept in
    ``self.episodes``; ``save_dir`` writes them as .npz).  wandb / imageio / pygame are not
    required."""

    def __init__(self, venv, record_interval=-1, indices=(0,), sprite_dir=None, ascii_only=False,
                 on_episode=None, save_dir=None):
        self.env = venv
        self.num_envs = venv.num_envs
        self.record_interval = int(record_interval)
        self.indices = [int(i) for i in indices]
        self.episode_counts = {i: 0 for i in self.indices}
        self.sprite_dir, self.ascii_only = sprite_dir, bool(ascii_only)
        self.on_episode, self.save_dir = on_episode, save_dir
        self._frames = {i: [] for i in self.indices}
        self.episodes = []

    def __getattr__(self, name):                   # gym.Wrapper-style pass-through
        return getattr(self.env, name)

    def _recording(self, i):
        return self.record_interval > 0 and self.episode_counts[i] % self.record_interval == 0

    def _frame(self, i):
        v = self.env.base_env(i)
        return str(v) if self.ascii_only else v.render_frame(self.sprite_dir)

    def reset(self):
        out = self.env.reset()
        for i in self.indices:
            self.episode_counts[i] += 1
            self._frames[i] = [self._frame(i)] if self._recording(i) else []
        return out

    def step(self, actions):
        obs, rew, dones, infos = self.env.step(actions)
        for i in self.indices:
            if dones[i]:
                # the env was auto-reset inside the kernel: its view shows the first frame of the
                # next episode, which starts that episode's recording
                if self._frames[i]:
                    ep = (i, self.episode_counts[i], self._frames[i])
                    if self.on_episode is not None:
                        self.on_episode(*ep)
                    else:
                        self.episodes.append(ep)
                    if self.save_dir and not self.ascii_only:
                        os.makedirs(self.save_dir, exist_ok=True)
                        np.savez_compressed(os.path.join(self.save_dir, "env%d_ep%d.npz" % (i, ep[1])),
                                            frames=np.stack(ep[2]))
                self.episode_counts[i] += 1
                self._frames[i] = []
            if self._recording(i):
                self._frames[i].append(self._frame(i))
        return obs, rew, dones, infos
