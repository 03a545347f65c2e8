"""The players an ``OvercookedVecEnv`` seats (see ``vec_env`` for the overview): ``RandomPartner``,
``MLPPolicy``, ``MLPActorCritic``, ``LSTMActorCritic``, ``TorchPolicyPartner``, ``RecurrentPolicyPartner``,
``FusedMLPPartner``, ``FusedActorCriticPartner``, ``FusedRecurrentPartner``."""
import ctypes

import numpy as np
import torch

from . import _lib
from .batched import OBS_KEYS, OBS_TYPE, pcg32_seed_states


def rows_and_timestep(obs):
    """(feature-major rows [F][n], timestep [n]) of an observation: an ``ObsView``'s own storage,
    or -- an observation dict without ``rows`` (any other env) -- concatenated the slow way."""
    rows = getattr(obs, "rows", None)
    if rows is None:
        rows = torch.cat([obs[k].reshape(obs[k].shape[0], -1) for k in OBS_KEYS], dim=1).T
    ts = getattr(obs, "timestep", None)
    return rows, ts if ts is not None else obs["timestep"].reshape(-1)


class _Seat:
    """What the players built on ``act_into(obs, move_row, comm_row)`` share."""
    sample = False

    def _pick(self, logits, dim):
        if self.sample:     # argmax(logits - log E), E ~ Exp(1)  ==  a categorical sample
            logits = logits - torch.empty_like(logits).exponential_().log_()
        return logits.argmax(dim=dim)

    def __call__(self, obs):
        n = next(iter(obs.values())).shape[0]
        out = torch.empty((2, n), dtype=torch.int32, device=self.device)
        self.act_into(obs, out[0], out[1])
        return out.T


class RandomPartner(_Seat):
    """Uniform random partner (move 0..3, comm 0..C-1) from a PCG32 stream per env.  In the
    partner seat of an ``OvercookedVecEnv`` it costs NO launch: the fused step kernel draws the
    actions itself (``oc_step_opts.alt_rng``, include/oc_hip.h) and reports them in action rows
    2, 3.  Anywhere else (``act_into`` / call) it is one launch of ``oc_random_actions``."""
    graph_safe = True
    in_kernel = True            # OvercookedVecEnv hands `rng_state(n)` to the step kernel

    def __init__(self, num_comm, seed=0, device="cuda"):
        self.C = int(num_comm)
        self.seed = int(seed)
        self.device = torch.device(device)
        self._L = _lib.load()
        self._rng = None

    def rng_state(self, n):
        """int32 [n] tensor holding the n PCG32 states (uint32 bit patterns)."""
        return self._state(n)

    def _state(self, n):
        if self._rng is None or self._rng.numel() != n:
            self._rng = pcg32_seed_states(self.seed, (n,), self.device)
        return self._rng

    def act_into(self, obs, move_row, comm_row):
        n = move_row.numel()
        _lib.call(self._L, "oc_random_actions", move_row.device.index, self._state(n).data_ptr(),
                  move_row.data_ptr(), comm_row.data_ptr(), self.C, n)

    def get_state(self, n):
        """A copy of the generator state for n envs (allocated on first use)."""
        return self._state(n).clone()

    def set_state(self, st):
        self._state(st.numel()).copy_(st)


class MLPPolicy(torch.nn.Module):
    """A small two-layer policy over get_observation2's 22 + S + 2C features (+ timestep):
    returns (move logits [4][n], comm logits [C][n]).  Feature-major on purpose: the kernel
    leaves a viewer's observation as [F][n] rows in HBM (float32 with ``obs_dtype=float32``), so
    the first layer is one GEMM on those rows as they lie -- no gather, no transpose, no concat.
    An observation dict without ``rows`` (any other env) is concatenated the slow way."""
    feature_major = True

    def __init__(self, num_subtasks, num_comm, hidden=64, seed=0):
        super().__init__()
        F = 22 + int(num_subtasks) + 2 * int(num_comm)
        g = torch.Generator().manual_seed(int(seed))
        init = lambda *shape: torch.nn.Parameter(
            (torch.rand(shape, generator=g) * 2 - 1) / float(np.sqrt(shape[-1])))
        self.w1, self.b1, self.wt = init(hidden, F), init(hidden, 1), init(hidden, 1)
        self.w2, self.b2 = init(4 + int(num_comm), hidden), init(4 + int(num_comm), 1)
        self.C = int(num_comm)
        self._more_parameters(init, hidden)

    def _more_parameters(self, init, hidden):
        """A subclass draws its own parameters here: from the same generator, after these."""

    def _hidden(self, obs):
        """tanh of the first layer, [H][n]."""
        rows, ts = rows_and_timestep(obs)
        ts = ts.unsqueeze(0)
        if rows.dtype != torch.float32:
            rows = rows.to(torch.float32)
        h = torch.addmm(self.b1, self.w1, rows)                 # [H][n]
        h = torch.addcmul(h, self.wt, ts.to(torch.float32))
        return torch.tanh_(h)

    def forward(self, obs):
        out = torch.addmm(self.b2, self.w2, self._hidden(obs))  # [4 + C][n]
        return out[:4], out[4:]


class MLPActorCritic(MLPPolicy):
    """``MLPPolicy`` with a value head on the same hidden layer: ``value = wv . tanh(h) + bv``.  The
    head's parameters are drawn after the parent's, so ``MLPActorCritic(S, C, seed=s)`` carries the
    policy weights of ``MLPPolicy(S, C, seed=s)``; ``forward`` is the parent's."""

    def _more_parameters(self, init, hidden):
        self.wv, self.bv = init(1, hidden), init(1, 1)

    def forward_ac(self, obs):
        """(move logits [4][n], comm logits [C][n], value [n])."""
        h = self._hidden(obs)
        out = torch.addmm(self.b2, self.w2, h)                  # [4 + C][n]
        return out[:4], out[4:], torch.addmm(self.bv, self.wv, h).reshape(-1)


class LSTMActorCritic(torch.nn.Module):
    """One LSTM cell of 64 units with the actor's and the critic's heads on its output: the network of
    include/oc_policy.h's recurrent-seat section in plain float32, gates in ``torch.nn.LSTMCell``'s order i, f, g, o.

        forward(obs, state, episode_start) -> (move logits [4][n], comm logits [C][n], (h, c), value [n])

    The logits are feature-major, as ``MLPPolicy``'s.  ``state`` = (h, c), float32 [n][64] each: env-major,
    which is what ``RecurrentPolicyPartner``'s protocol asks of a state (``initial_state(n)`` gives one); the
    fused seat keeps the same numbers transposed, [64][n].  ``episode_start`` float [n] (or None): where it is
    > 0 the env starts from the zero state, by a select.  ``FusedRecurrentPartner`` runs the same weights as
    one launch.  Parameters, drawn by ``MLPPolicy``'s rule from one generator in this order: wx [256][F],
    wt [256][1], b [256][1], wh [256][64], w2 [4 + C][64], b2 [4 + C][1], wv [1][64], bv [1][1]."""
    feature_major = True
    hidden = 64

    def __init__(self, num_subtasks, num_comm, seed=0):
        super().__init__()
        F, H = 22 + int(num_subtasks) + 2 * int(num_comm), self.hidden
        g = torch.Generator().manual_seed(int(seed))
        init = lambda *shape: torch.nn.Parameter(
            (torch.rand(shape, generator=g) * 2 - 1) / float(np.sqrt(shape[-1])))
        self.wx, self.wt, self.b, self.wh = init(4 * H, F), init(4 * H, 1), init(4 * H, 1), init(4 * H, H)
        self.w2, self.b2 = init(4 + int(num_comm), H), init(4 + int(num_comm), 1)
        self.wv, self.bv = init(1, H), init(1, 1)
        self.C = int(num_comm)

    def initial_state(self, n, device=None):
        """(h, c) of n envs that have not started: zeros [n][64]."""
        dev = device if device is not None else self.wx.device
        return (torch.zeros((n, self.hidden), dtype=torch.float32, device=dev),
                torch.zeros((n, self.hidden), dtype=torch.float32, device=dev))

    def forward(self, obs, state, episode_start=None):
        rows, ts = rows_and_timestep(obs)
        dt = self.wx.dtype                                          # float32 (float64 after .double(): the tests)
        if rows.dtype != dt:
            rows = rows.to(dt)
        h, c = state[0].T, state[1].T                               # [64][n] views
        if episode_start is not None:
            s = (episode_start > 0).unsqueeze(0)
            h, c = torch.where(s, torch.zeros_like(h), h), torch.where(s, torch.zeros_like(c), c)
        z = torch.addmm(self.b, self.wx, rows)                      # [256][n]
        z = torch.addcmul(z, self.wt, ts.to(dt).unsqueeze(0))
        z = torch.addmm(z, self.wh, h)
        i, f, g, o = z.view(4, self.hidden, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out = torch.addmm(self.b2, self.w2, h)                      # [4 + C][n]
        return out[:4], out[4:], (h.T, c.T), torch.addmm(self.bv, self.wv, h).reshape(-1)


class TorchPolicyPartner(_Seat):
    """A torch module in the partner (or ego) seat.  ``policy(obs) -> (move_logits,
    comm_logits)``, each [n, k] -- or [k, n] when ``policy.feature_major`` is true.  Actions are
    the argmax (``sample=False``) or a categorical sample (Gumbel-max on the default CUDA
    generator, so the draw is hipGraph-capturable), written straight into the kernel's action
    rows.  ``update(rewards, dones)`` -- pantheonrl's ``Agent.update`` -- is forwarded to
    ``on_update`` (e.g. a rollout buffer's add), called after every step."""

    def __init__(self, policy, sample=True, seed=None, device="cuda", on_update=None):
        self.policy = policy
        self.sample = bool(sample)
        self.device = torch.device(device)
        self.on_update = on_update
        # stateless between steps and fixed-shape => one capture serves every later step
        self.graph_safe = on_update is None
        if seed is not None:
            with torch.cuda.device(self.device):
                torch.cuda.manual_seed(int(seed))

    @torch.no_grad()
    def act_into(self, obs, move_row, comm_row):
        mv, cm = self.policy(obs)
        dim = 0 if getattr(self.policy, "feature_major", False) else 1
        move_row.copy_(self._pick(mv, dim))
        comm_row.copy_(self._pick(cm, dim))

    def update(self, rewards, dones):
        if self.on_update is not None:
            self.on_update(rewards, dones)


class _RecordingSeat(_Seat):
    """What the two seats that record a rollout share: ``episode_start`` / ``value`` tensors, an optional
    ``sink`` (a ``RolloutSink``) and an optional host-side ``on_update`` hook."""
    sink = on_update = None

    def update(self, rewards, dones):
        """pantheonrl's ``Agent.update(reward, done)`` for the batch: ``dones`` become the next
        step's ``episode_start`` (agents.py:207-208), the reward joins the recorded transition."""
        self.episode_start.copy_(dones)
        if self.sink is not None:
            self.sink.add_reward(rewards, dones)
        if self.on_update is not None:
            self.on_update(rewards, dones)

    def finish_rollout(self, gamma=0.99, gae_lambda=0.95):
        """What ``OnPolicyAgent.get_action`` does on a full buffer before ``train()`` (agents.py:127-131):
        ``buf.compute_returns_and_advantage(last_values=self.values, dones=self._last_episode_starts[0])``
        with the values of the last ``act_into`` and the last ``done`` row.  Returns the sink's
        (advantages, returns); the sink is NOT reset -- the caller does that after its update
        (agents.py:158)."""
        if self.sink is None:
            raise ValueError("finish_rollout needs a sink")
        return self.sink.compute_returns_and_advantage(self.value, self.episode_start, gamma, gae_lambda)


class RecurrentPolicyPartner(_RecordingSeat):
    """A STATEFUL torch policy in the partner (or ego) seat: the batched form of what the
    reference seats there -- ``OnPolicyAgent(RecurrentPPO('MultiInputPolicy', ...))``
    (trainer.py:92-112; pantheonrl/common/agents.py:112-214; sb3_contrib's recurrent policies
    carry LSTM states per env and reset them where ``episode_starts`` is set).

        policy(obs, state, episode_start) -> (move_logits, comm_logits, new_state[, value])

    ``obs``: the viewer's ``ObsView`` ([n, k] keys, ``rows`` [F][n], ``timestep``); ``state``: a
    tuple of ``[n, ...]`` tensors OWNED BY THE PARTNER (updated in place, so a captured graph keeps
    their addresses); ``episode_start``: float32 [n], 1 where the env's previous step returned done
    (the step kernel's ``done`` row, handed over by ``update``) and for every env on the first step
    after a reset -- SB3's ``_last_episode_starts``.  With ``mask_state`` (default) the partner
    itself puts the initial state back into the rows of starting envs before the call, so a policy
    that ignores ``episode_start`` is still correct.  Logits are ``[n, k]``, or ``[k, n]`` when
    ``policy.feature_major``; ``value`` is optional ([n] or [n, 1]).

    Actions: argmax, or a categorical sample (Gumbel-max on the default CUDA generator:
    hipGraph-capturable), written into the kernel's action rows; their log-probability under the
    policy is computed either way.  ``sink`` (a ``RolloutSink``) records (obs, action, log_prob,
    value, episode_start) at ``act_into`` and (reward, done) at ``update`` WITHOUT leaving the
    device or the graph; ``on_update(rewards, dones)`` is the host-side learner hook (it switches
    graph capture off, as for ``TorchPolicyPartner``)."""

    def __init__(self, policy, state, sample=True, seed=None, device="cuda", sink=None, on_update=None,
                 mask_state=True):
        self.policy = policy
        self.sample = bool(sample)
        self.device = torch.device(device)
        self.sink = sink
        self.on_update = on_update
        self.mask_state = bool(mask_state)
        self.graph_safe = on_update is None
        state = tuple(state) if isinstance(state, (tuple, list)) else (state,)
        self.initial = tuple(s.detach().clone().to(self.device) for s in state)
        self.state = tuple(s.clone() for s in self.initial)
        n = self.state[0].shape[0]
        self.episode_start = torch.ones(n, dtype=torch.float32, device=self.device)
        self.log_prob = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.value = torch.zeros(n, dtype=torch.float32, device=self.device)
        if seed is not None:
            with torch.cuda.device(self.device):
                torch.cuda.manual_seed(int(seed))

    def reset(self):
        """A fresh rollout: every env starts an episode (called by ``reset_tensors``)."""
        self.episode_start.fill_(1.0)
        for s, s0 in zip(self.state, self.initial):
            s.copy_(s0)

    @torch.no_grad()
    def act_into(self, obs, move_row, comm_row):
        es = self.episode_start
        if self.mask_state:
            for s, s0 in zip(self.state, self.initial):
                s.copy_(torch.where(es.view((-1,) + (1,) * (s.dim() - 1)) > 0, s0, s))
        out = self.policy(obs, self.state, es)
        mv, cm, new_state = out[0], out[1], out[2]
        value = out[3] if len(out) > 3 else None
        dim = 0 if getattr(self.policy, "feature_major", False) else 1
        a_mv, a_cm = self._pick(mv, dim), self._pick(cm, dim)
        lp = (torch.log_softmax(mv.float(), dim=dim).gather(dim, a_mv.unsqueeze(dim)).squeeze(dim)
              + torch.log_softmax(cm.float(), dim=dim).gather(dim, a_cm.unsqueeze(dim)).squeeze(dim))
        move_row.copy_(a_mv)
        comm_row.copy_(a_cm)
        self.log_prob.copy_(lp)
        if value is not None:
            self.value.copy_(value.reshape(-1))
        new_state = tuple(new_state) if isinstance(new_state, (tuple, list)) else (new_state,)
        for s, ns in zip(self.state, new_state):
            s.copy_(ns)
        if self.sink is not None:
            rows, ts = rows_and_timestep(obs)
            self.sink.add(rows, ts, move_row, comm_row, lp, value, es)

    def get_state(self, n=None):
        return (tuple(s.clone() for s in self.state), self.episode_start.clone(), self.log_prob.clone(),
                self.value.clone(), None if self.sink is None else self.sink.get_state())

    def set_state(self, st):
        for s, v in zip(self.state, st[0]):
            s.copy_(v)
        self.episode_start.copy_(st[1])
        self.log_prob.copy_(st[2])
        self.value.copy_(st[3])
        if self.sink is not None:
            self.sink.set_state(st[4])


def _f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def pack_fragments(L, policy, value_head=False):
    """The module's current weights in MFMA fragment order (include/oc_policy.h: the packers of ``L``,
    the policy library): numpy ``(o1, o2, ob)`` = first layer (timestep column and bias folded in),
    second layer, second bias.  ``value_head``: an ``MLPActorCritic``'s value row rides in ``o2`` / ``ob``
    (``oc_policy_pack_w2v`` / ``_b2v``).  Host code only: no device call."""
    F, C = int(policy.w1.shape[1]), int(policy.C)
    w1, wt, b1, w2, b2 = (_f32(t) for t in (policy.w1, policy.wt, policy.b1, policy.w2, policy.b2))
    o1 = np.zeros((2, L.oc_policy_ksteps(F), 64, 8), np.uint16)
    o2 = np.zeros((4, 64, 8), np.uint16)
    ob = np.zeros((64, 16), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    done = [(L.oc_policy_pack_w1(_fp(w1), _fp(wt.reshape(-1)), _fp(b1.reshape(-1)), F, vp(o1)), "oc_policy_pack_w1")]
    if value_head:
        wv, bv = _f32(policy.wv).reshape(-1), _f32(policy.bv).reshape(-1)
        done += [(L.oc_policy_pack_w2v(_fp(w2), _fp(wv), C, vp(o2)), "oc_policy_pack_w2v"),
                 (L.oc_policy_pack_b2v(_fp(b2.reshape(-1)), _fp(w2), _fp(bv), _fp(wv), C, _fp(ob)), "oc_policy_pack_b2v")]
    else:
        done += [(L.oc_policy_pack_w2(_fp(w2), C, vp(o2)), "oc_policy_pack_w2"),
                 (L.oc_policy_pack_b2(_fp(b2.reshape(-1)), _fp(w2), C, _fp(ob)), "oc_policy_pack_b2")]
    for rc, what in done:
        _lib.check(rc, what, L)
    return o1, o2, ob


def pack_w2t(L, policy):
    """A learner's own image of an ``MLPActorCritic``'s second layer (include/oc_policy.h: ``w2t``): numpy
    float32 [2][16][64], the folded weights transposed.  Host code only, as ``pack_fragments``."""
    out = np.zeros((2, 16, 64), np.float32)
    rc = L.oc_policy_pack_w2t(_fp(_f32(policy.w2)), _fp(_f32(policy.wv).reshape(-1)), int(policy.C), _fp(out))
    _lib.check(rc, "oc_policy_pack_w2t", L)
    return out


def _stream_seed(seed):
    """The PCG32 stream seed of a fused seat.  None: a different default per seat built (two seats left at
    their defaults -- an ego and a partner -- must not share per-env random streams: their samples would
    use the same uniform draw every step); pass a seed for a reproducible stream."""
    if seed is None:
        seed = 0x5EED + 1000003 * FusedMLPPartner._seats
    FusedMLPPartner._seats += 1
    return int(seed)


def _upload(held, arrays, device):
    """Packed numpy images on the device.  ``held`` None: fresh tensors; otherwise copied into ``held`` in
    place: a captured graph keeps the addresses."""
    new = tuple(torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device) for a in arrays)
    if held is None:
        return new
    for old, cur in zip(held, new):
        old.copy_(cur)
    return held


class _FusedSeat:
    """What the two seats of the hand-written policy kernel share: the checks of the module, the
    default stream seed, the packed weights ``_w`` (three device tensors whose addresses never change:
    ``weight_ptrs()``) and ``refresh()``."""
    graph_safe = True
    _module = _module_error = None      # the module class a seat runs, and what it says to any other
    _value_head = False

    def __init__(self, policy, sample, seed, device, keep_logits):
        seed = _stream_seed(seed)
        if not isinstance(policy, self._module):
            raise TypeError(self._module_error)
        if policy.w1.shape[0] != 64:
            raise ValueError("the fused kernel has 64 hidden units (got %d)" % policy.w1.shape[0])
        if not 1 <= policy.C <= 16:
            raise ValueError("the fused kernel samples at most 16 comm channels (got %d)" % policy.C)
        self.policy, self.sample, self.seed = policy, bool(sample), int(seed)
        self.device = torch.device(device)
        self.keep_logits = bool(keep_logits)
        self._L = _lib.load(lib="policy")
        self.F = int(policy.w1.shape[1])
        self.C = int(policy.C)
        self._w = None
        self.refresh()

    def refresh(self):
        """(Re)pack the module's current weights into MFMA fragment order and upload them."""
        self._w = _upload(self._w, pack_fragments(self._L, self.policy, self._value_head), self.device)

    def weight_ptrs(self):
        """Device addresses of the three fragment tensors (w1, w2, b2)."""
        w = self._w
        return w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr()

    @property
    def weight_device(self):
        """Where the fragment tensors live (``device`` with its index resolved)."""
        return self._w[0].device

    def _check_rows(self, rows):
        if rows.shape[0] != self.F:
            raise ValueError("the policy was built for %d observation rows, the env has %d" % (self.F, rows.shape[0]))


class FusedMLPPartner(_FusedSeat):
    """An ``MLPPolicy`` in the partner (or ego) seat as ONE launch of the hand-written policy
    kernel (include/oc_policy.h, csrc/oc_policy.hip): both products on the matrix cores
    (v_mfma_f32_32x32x16_f16, one wave = 32 envs, the hidden layer never leaves the accumulator
    registers), tanh, a categorical sample from two PCG32 streams per env, and the result written as
    the int32 [n][2] (move, comm) pairs the step kernel consumes as they lie.  What
    ``TorchPolicyPartner(MLPPolicy(...))`` does in ~12 torch launches.  Two of them (ego + partner)
    share one launch (``FusedMLPPartner.launch``).  Weights are packed once (``refresh()`` after an
    optimiser step); fp16 operands, fp32 accumulation: logits within 2e-2 of the fp32 module's."""
    _seats = 0          # fused seats built so far: the default stream seed differs from seat to seat
    _module = MLPPolicy
    _module_error = "FusedMLPPartner runs gym_comm_amd.vec_env.MLPPolicy; wrap any other module in TorchPolicyPartner"

    def __init__(self, policy, sample=True, seed=None, device="cuda", keep_logits=False):
        self._rng = self.pairs = self.logits = None
        super().__init__(policy, sample, seed, device, keep_logits)

    def _buffers(self, n):
        if self.pairs is None or self.pairs.shape[0] != n:
            self._rng = pcg32_seed_states(self.seed, (2, n), self.device)
            self.pairs = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
            self.logits = (torch.zeros((4 + self.C, n), dtype=torch.float32, device=self.device)
                           if self.keep_logits else None)

    def _player(self, rows):
        self._check_rows(rows)
        self._buffers(rows.shape[1])
        return _lib.PolicyPlayer(rows.data_ptr(), *self.weight_ptrs(), self._rng.data_ptr() if self.sample else None,
                                 self.pairs.data_ptr(), self.logits.data_ptr() if self.logits is not None else None)

    @staticmethod
    def launch(players, rows, timestep):
        """One launch for one or two FusedMLPPartner, each on its own observation rows ([F][n]
        views of the env's obs tensor); their ``pairs`` tensors hold the result."""
        first = players[0]
        if any(pl.F != first.F or pl.C != first.C for pl in players):
            raise ValueError("players of one launch share F and C")
        arr = (_lib.PolicyPlayer * len(players))(*[pl._player(r) for pl, r in zip(players, rows)])
        _lib.call(first._L, "oc_policy_mlp", rows[0].device.index, arr, len(players), timestep.data_ptr(),
                  first.F, first.C, OBS_TYPE[rows[0].dtype], rows[0].shape[1])

    _PCG_MULT, _PCG_INC = 747796405, 2891336453          # csrc/oc_policy_device.h: pcg32
    _PCG_MULT_INV = pow(747796405, -1, 1 << 32)

    def rewind_rng(self):
        """Step both PCG32 streams of every env back by ONE draw (the generator's state update is
        an invertible affine map mod 2^32): the next evaluation repeats the last one's draw.  How a
        one-launch closed loop re-primes after a reset without leaving the sequence the two-launch
        form walks (``ClosedLoop.prime``)."""
        if self._rng is None or not self.sample:
            return
        s = self._rng.to(torch.int64) & 0xFFFFFFFF
        s = ((s - self._PCG_INC) * self._PCG_MULT_INV) & 0xFFFFFFFF
        self._rng.copy_(torch.where(s >= (1 << 31), s - (1 << 32), s).to(torch.int32))

    def step_policy(self, n):
        """(w1, w2, b2, rng) device addresses for oc_step_opts.policy (the step kernel evaluates
        this policy itself; its result lands in ``self.pairs``)."""
        self._buffers(n)
        return (*self.weight_ptrs(), self._rng.data_ptr() if self.sample else None)

    def pairs_for(self, obs):
        """obs: an ``ObsView`` of the env (``rows`` [F][n], ``timestep``).  Returns int32 [n][2]."""
        FusedMLPPartner.launch([self], [obs.rows], obs.timestep)
        return self.pairs

    def act_into(self, obs, move_row, comm_row):       # the generic partner protocol (two more copies)
        pr = self.pairs_for(obs)
        move_row.copy_(pr[:, 0])
        comm_row.copy_(pr[:, 1])

    def __call__(self, obs):
        return self.pairs_for(obs)

    def get_state(self, n):
        """The player's mutable state: its random streams and its pairs (in a one-launch closed
        loop the pairs are the NEXT step's actions, i.e. state)."""
        self._buffers(n)
        return self._rng.clone(), self.pairs.clone()

    def set_state(self, st):
        self._rng.copy_(st[0])
        self.pairs.copy_(st[1])


class FusedActorCriticPartner(_FusedSeat, _RecordingSeat):
    """An ``MLPActorCritic`` in the seat of a player that LEARNS, as ONE launch of the policy kernel's
    actor-critic form (include/oc_policy.h: ``oc_policy_mlp_ac``): what ``OnPolicyAgent.get_action``
    takes from its forward (pantheonrl/common/agents.py:112-194) -- the sampled action, written into
    the env's action rows as they lie, its log-probability and the state's value -- and, with a
    ``sink`` (a ``RolloutSink``), the recording of the step behind it.  The value head rides in a row
    of the second matrix product that no logit uses; the log-probability comes from the softmax
    normaliser the sampler forms anyway.

    The seat protocol is ``RecurrentPolicyPartner``'s: ``act_into``, ``update(rewards, dones)``
    (``dones`` become the next step's ``episode_start``, the reward joins the recorded step),
    ``reset()``, ``finish_rollout()``.  Not a ``FusedMLPPartner``: the paths ``vec_env`` gives that
    class (pairs consumed as they lie, the step kernel evaluating the policy itself) produce
    neither value nor log-probability.  ``score(obs, pairs)`` evaluates GIVEN actions: what a
    learner's update needs."""
    _module = MLPActorCritic
    _module_error = "FusedActorCriticPartner runs gym_comm_amd.vec_env.MLPActorCritic"
    _value_head = True          # refresh() packs the value row too

    def __init__(self, policy, sample=True, seed=None, device="cuda", sink=None, keep_logits=False):
        self.sink = sink
        self._rng = self.episode_start = self.log_prob = self.value = self.logits = None
        super().__init__(policy, sample, seed, device, keep_logits)

    def _buffers(self, n):
        if self.log_prob is None or self.log_prob.numel() != n:
            dev = self.device
            self._rng = pcg32_seed_states(self.seed, (2, n), dev)
            self.episode_start = torch.ones(n, dtype=torch.float32, device=dev)
            self.log_prob = torch.zeros(n, dtype=torch.float32, device=dev)
            self.value = torch.zeros(n, dtype=torch.float32, device=dev)
            self.logits = torch.zeros((4 + self.C, n), dtype=torch.float32, device=dev) if self.keep_logits else None

    def _launch(self, rows, timestep, given, move_row, comm_row, log_prob, value):
        n = rows.shape[1]
        self._check_rows(rows)
        if not rows.is_contiguous():
            raise ValueError("the kernel reads the observation rows as they lie: [F][n], contiguous")
        ptr = lambda t: None if t is None else t.data_ptr()
        use_rng = self.sample and given is None
        pl = _lib.PolicyAcPlayer(
            _lib.PolicyPlayer(rows.data_ptr(), *self.weight_ptrs(), self._rng.data_ptr() if use_rng else None, None,
                              ptr(self.logits) if given is None else None),
            ptr(given), ptr(move_row), ptr(comm_row), ptr(log_prob), ptr(value))
        _lib.call(self._L, "oc_policy_mlp_ac", rows.device.index, ctypes.byref(pl), 1, timestep.data_ptr(),
                  self.F, self.C, OBS_TYPE[rows.dtype], n)

    @staticmethod
    def _action_row(t, n):
        if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
            raise ValueError("an action row is a contiguous int32 tensor of %d elements" % n)
        return t

    def act_into(self, obs, move_row, comm_row):
        """ONE launch: the actions into ``move_row`` / ``comm_row`` (the env's own rows, no copy),
        ``self.log_prob`` and ``self.value``; then the sink's ``add``."""
        rows, ts = rows_and_timestep(obs)
        n = rows.shape[1]
        self._buffers(n)
        self._launch(rows, ts, None, self._action_row(move_row, n), self._action_row(comm_row, n),
                     self.log_prob, self.value)
        if self.sink is not None:
            self.sink.add(rows, ts, move_row, comm_row, self.log_prob, self.value, self.episode_start)

    def score(self, obs, pairs):
        """(log_prob [n], value [n]) of GIVEN actions, int32 [n][2] (move, comm), under the current
        weights: one launch, fresh tensors.  n is the scored batch's own (a minibatch of recorded
        rows, say), whatever the seat's: none of the seat's state -- streams, ``episode_start``,
        ``log_prob``, ``value``, kept logits -- is read, written or reallocated.  An index outside
        its head's range yields -inf."""
        rows, ts = rows_and_timestep(obs)
        n = rows.shape[1]
        if pairs.dtype != torch.int32 or tuple(pairs.shape) != (n, 2) or not pairs.is_contiguous():
            raise ValueError("pairs: a contiguous int32 [%d][2] tensor" % n)
        lp = torch.empty(n, dtype=torch.float32, device=rows.device)
        val = torch.empty(n, dtype=torch.float32, device=rows.device)
        self._launch(rows, ts, pairs, None, None, lp, val)
        return lp, val

    def reset(self):
        """A fresh rollout: every env starts an episode (called by ``reset_tensors``)."""
        if self.episode_start is not None:
            self.episode_start.fill_(1.0)

    def update(self, rewards, dones):
        """pantheonrl's ``Agent.update(reward, done)`` for the batch, on buffers that exist by now."""
        self._buffers(dones.numel())
        super().update(rewards, dones)

    def get_state(self, n):
        """The seat's mutable state: its random streams, ``episode_start``, the last ``log_prob`` /
        ``value`` and the sink's position."""
        self._buffers(n)
        return (self._rng.clone(), self.episode_start.clone(), self.log_prob.clone(), self.value.clone(),
                None if self.sink is None else self.sink.get_state())

    def set_state(self, st):
        self._rng.copy_(st[0])
        self.episode_start.copy_(st[1])
        self.log_prob.copy_(st[2])
        self.value.copy_(st[3])
        if self.sink is not None:
            self.sink.set_state(st[4])


def pack_lstm(L, policy):
    """An ``LSTMActorCritic``'s current weights as the three images of include/oc_policy.h's recurrent-seat section:
    numpy ``(gates, head, head_bias)``.  Host code only, as ``pack_fragments``."""
    F, C = int(policy.wx.shape[1]), int(policy.C)
    wx, wt, b, wh, w2, b2, wv, bv = (_f32(t) for t in (policy.wx, policy.wt, policy.b, policy.wh, policy.w2,
                                                       policy.b2, policy.wv, policy.bv))
    og = np.zeros((4, 2, L.oc_policy_lstm_ksteps(F), 64, 8), np.uint16)
    oh = np.zeros((4, 64, 8), np.uint16)
    ob = np.zeros((64, 16), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for rc, what in (
            (L.oc_policy_lstm_pack_gates(_fp(wx), _fp(wt.reshape(-1)), _fp(b.reshape(-1)), _fp(wh), F, vp(og)),
             "oc_policy_lstm_pack_gates"),
            (L.oc_policy_lstm_pack_head(_fp(w2), _fp(wv.reshape(-1)), C, vp(oh)), "oc_policy_lstm_pack_head"),
            (L.oc_policy_lstm_pack_head_bias(_fp(b2.reshape(-1)), _fp(bv.reshape(-1)), C, _fp(ob)),
             "oc_policy_lstm_pack_head_bias")):
        _lib.check(rc, what, L)
    return og, oh, ob


def pack_lstm_bwd(L, policy):
    """A recurrent learner's own image of an ``LSTMActorCritic`` (include/oc_policy.h: ``bwd``): numpy float32, Wh and
    [W2; wv] transposed for the backward's products.  Host code only, as ``pack_fragments``."""
    out = np.zeros(L.oc_policy_rppo_pack_bwd_elems(), np.float32)
    rc = L.oc_policy_rppo_pack_bwd(_fp(_f32(policy.wh)), _fp(_f32(policy.w2)), _fp(_f32(policy.wv).reshape(-1)),
                                   int(policy.C), _fp(out))
    _lib.check(rc, "oc_policy_rppo_pack_bwd", L)
    return out


class FusedRecurrentPartner(_RecordingSeat):
    """An ``LSTMActorCritic`` in the seat of a recurrent player as ONE launch (include/oc_policy.h:
    ``oc_policy_lstm_ac``): the masked state, the cell (the 256 gate rows on the matrix cores, one wave = 32
    envs, the update lane-local), both heads, the sampled action written into the env's action rows as
    they lie, its log-probability and the value -- what ``RecurrentPolicyPartner(LSTMActorCritic(...))`` does
    in some forty torch launches.  fp16 operands, fp32 accumulation and state: logits within 1.5e-3 and value
    within 1.4e-3 of the float32 module's, step by step over a 60-step trajectory (measured, not a bound:
    tests/test_recurrent_seat_gpu.py).

    The seat protocol is ``FusedActorCriticPartner``'s: ``act_into`` (then the sink's ``add``), ``update``,
    ``reset()``, ``finish_rollout()``, ``refresh()`` after the weights changed, ``get_state`` / ``set_state``.
    The seat owns ``h``, ``c``, float32 [64][n], updated IN PLACE by the launch (a lane reads exactly the
    elements it writes); an env whose ``episode_start`` is set starts from the zero state inside the kernel.
    ``score(obs, state, episode_start, pairs)`` evaluates GIVEN actions from a GIVEN state and writes no
    state at all.  ``begin_rollout()`` (called where ``sink.reset()`` is called otherwise) keeps the state the
    rollout starts from in ``h0`` / ``c0``: what ``RecurrentPPOLearner`` (learner.py) unrolls the recorded
    sequences from.  With a sink that has a ``state_window`` W the seat also records ``h`` / ``c`` in front of every
    W-th step into ``sink.lstm_states`` (``oc_policy_window_snapshot``, one launch more per step): what the learner
    unrolls WINDOWS of W steps from."""
    graph_safe = True

    def __init__(self, policy, sample=True, seed=None, device="cuda", sink=None, keep_logits=False):
        seed = _stream_seed(seed)
        if not isinstance(policy, LSTMActorCritic):
            raise TypeError("FusedRecurrentPartner runs gym_comm_amd.vec_env.LSTMActorCritic; wrap any other module in "
                            "RecurrentPolicyPartner")
        if not 1 <= policy.C <= 16:
            raise ValueError("the fused kernel samples at most 16 comm channels (got %d)" % policy.C)
        self.policy, self.sample, self.seed = policy, bool(sample), int(seed)
        self.device = torch.device(device)
        self.sink = sink
        self.keep_logits = bool(keep_logits)
        self._L = _lib.load(lib="policy")
        self.F, self.C = int(policy.wx.shape[1]), int(policy.C)
        if self.F + 2 > 64:
            raise ValueError("the fused kernel takes at most 62 observation rows (got %d)" % self.F)
        self._rng = self.episode_start = self.log_prob = self.value = self.logits = self.h = self.c = None
        self.h0 = self.c0 = None
        self._w = None
        self.refresh()

    def refresh(self):
        """(Re)pack the module's current weights and upload them, in place after the first time."""
        self._w = _upload(self._w, pack_lstm(self._L, self.policy), self.device)

    def weight_ptrs(self):
        """Device addresses of the three images (gates, head, head_bias)."""
        w = self._w
        return w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr()

    @property
    def weight_device(self):
        """Where the images live (``device`` with its index resolved)."""
        return self._w[0].device

    def _buffers(self, n):
        if self.log_prob is None or self.log_prob.numel() != n:
            dev = self.device
            self._rng = pcg32_seed_states(self.seed, (2, n), dev)
            self.episode_start = torch.ones(n, dtype=torch.float32, device=dev)
            self.log_prob = torch.zeros(n, dtype=torch.float32, device=dev)
            self.value = torch.zeros(n, dtype=torch.float32, device=dev)
            self.h = torch.zeros((64, n), dtype=torch.float32, device=dev)
            self.c = torch.zeros((64, n), dtype=torch.float32, device=dev)
            self.h0, self.c0 = torch.zeros_like(self.h), torch.zeros_like(self.c)
            self.logits = torch.zeros((4 + self.C, n), dtype=torch.float32, device=dev) if self.keep_logits else None

    def _launch(self, rows, timestep, state_in, state_out, episode_start, given, move_row, comm_row, log_prob, value):
        n = rows.shape[1]
        if rows.shape[0] != self.F:
            raise ValueError("the policy was built for %d observation rows, the env has %d" % (self.F, rows.shape[0]))
        if not rows.is_contiguous():
            raise ValueError("the kernel reads the observation rows as they lie: [F][n], contiguous")
        for t in tuple(state_in) + tuple(t for t in state_out if t is not None):
            if t.dtype != torch.float32 or tuple(t.shape) != (64, n) or not t.is_contiguous():
                raise ValueError("a state tensor is contiguous float32 [64][%d]" % n)
        if episode_start is not None and (episode_start.dtype != torch.float32 or episode_start.numel() != n
                                          or not episode_start.is_contiguous()):
            raise ValueError("episode_start: a contiguous float32 tensor of %d elements" % n)
        ptr = lambda t: None if t is None else t.data_ptr()
        use_rng = self.sample and given is None
        w = self._w
        pl = _lib.PolicyLstmPlayer(
            rows.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), state_in[0].data_ptr(),
            state_in[1].data_ptr(), ptr(state_out[0]), ptr(state_out[1]), ptr(episode_start),
            self._rng.data_ptr() if use_rng else None, ptr(given), None, ptr(move_row), ptr(comm_row), ptr(log_prob),
            ptr(value), ptr(self.logits) if given is None else None)
        _lib.call(self._L, "oc_policy_lstm_ac", rows.device.index, ctypes.byref(pl), timestep.data_ptr(),
                  self.F, self.C, OBS_TYPE[rows.dtype], n)

    def act_into(self, obs, move_row, comm_row):
        """ONE launch: the actions into ``move_row`` / ``comm_row`` (the env's own rows, no copy),
        ``self.log_prob``, ``self.value`` and the new ``self.h`` / ``self.c``; then the sink's ``add``.  A sink with a
        ``state_window`` gets one launch more, in front: the snapshot of ``h`` / ``c`` into its ``lstm_states``."""
        rows, ts = rows_and_timestep(obs)
        n = rows.shape[1]
        self._buffers(n)
        row = FusedActorCriticPartner._action_row
        state = (self.h, self.c)
        sink = self.sink
        if sink is not None and getattr(sink, "state_window", None) is not None:
            # the state BEFORE this step, kept where a window begins (one launch; it copies on every W-th slot only)
            if tuple(sink.lstm_states.shape[2:]) != (64, n):
                raise ValueError("the sink records states of %d envs, the seat steps %d" % (sink.lstm_states.shape[3], n))
            _lib.call(self._L, "oc_policy_window_snapshot", rows.device.index, sink.pos.data_ptr(), sink.n_steps,
                      sink.state_window, self.h.data_ptr(), self.c.data_ptr(), sink.lstm_states.data_ptr(), n)
        self._launch(rows, ts, state, state, self.episode_start, None, row(move_row, n), row(comm_row, n),
                     self.log_prob, self.value)
        if self.sink is not None:
            self.sink.add(rows, ts, move_row, comm_row, self.log_prob, self.value, self.episode_start)

    def score(self, obs, state, episode_start, pairs):
        """(log_prob [n], value [n]) of GIVEN actions, int32 [n][2] (move, comm), from the GIVEN ``state`` =
        (h, c), float32 [64][n], and ``episode_start`` (float32 [n], or None) under the current weights: one
        launch, fresh tensors.  n is the scored batch's own; neither ``state`` nor anything of the seat --
        its own state, streams, ``episode_start``, ``log_prob``, ``value``, kept logits -- is written.  An
        index outside its head's range yields -inf."""
        rows, ts = rows_and_timestep(obs)
        n = rows.shape[1]
        if pairs.dtype != torch.int32 or tuple(pairs.shape) != (n, 2) or not pairs.is_contiguous():
            raise ValueError("pairs: a contiguous int32 [%d][2] tensor" % n)
        lp = torch.empty(n, dtype=torch.float32, device=rows.device)
        val = torch.empty(n, dtype=torch.float32, device=rows.device)
        self._launch(rows, ts, tuple(state), (None, None), episode_start, pairs, None, None, lp, val)
        return lp, val

    def reset(self):
        """A fresh rollout: every env starts an episode (called by ``reset_tensors``); the kernel's select
        then takes the zero state whatever ``h`` / ``c`` hold."""
        if self.episode_start is not None:
            self.episode_start.fill_(1.0)

    def begin_rollout(self, n=None):
        """A new rollout begins with the state as it is: ``h -> h0``, ``c -> c0`` (two device copies, no
        synchronisation) and the sink, if there is one, reset.  ``episode_start`` stays as it is.  ``n``: the
        number of envs, for a seat that has not acted yet (its state is zero)."""
        if self.h is None:
            if n is None and self.sink is not None:
                n = self.sink.obs.shape[2]
            if n is None:
                raise ValueError("begin_rollout before the first act_into needs the number of envs")
            self._buffers(int(n))
        self.h0.copy_(self.h)
        self.c0.copy_(self.c)
        if self.sink is not None:
            self.sink.reset()

    def update(self, rewards, dones):
        """pantheonrl's ``Agent.update(reward, done)`` for the batch, on buffers that exist by now."""
        self._buffers(dones.numel())
        super().update(rewards, dones)

    def get_state(self, n):
        """The seat's mutable state: its random streams, ``episode_start``, the last ``log_prob`` / ``value``,
        the sink's position, ``h`` and ``c``, and the rollout's start state ``h0`` and ``c0``."""
        self._buffers(n)
        return (self._rng.clone(), self.episode_start.clone(), self.log_prob.clone(), self.value.clone(),
                None if self.sink is None else self.sink.get_state(), self.h.clone(), self.c.clone(),
                self.h0.clone(), self.c0.clone())

    def set_state(self, st):
        self._rng.copy_(st[0])
        self.episode_start.copy_(st[1])
        self.log_prob.copy_(st[2])
        self.value.copy_(st[3])
        if self.sink is not None:
            self.sink.set_state(st[4])
        self.h.copy_(st[5])
        self.c.copy_(st[6])
        if len(st) > 7:                      # (a 7-tuple: a state taken before h0 / c0 existed)
            self.h0.copy_(st[7])
            self.c0.copy_(st[8])
