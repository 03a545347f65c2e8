"""``RolloutSink``: a partner's rollout buffer on the device (see ``vec_env`` for the overview)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .batched import OBS_TYPE


class RolloutSink:
    """What pantheonrl's ``OnPolicyAgent`` keeps per step in its rollout buffer -- ``buf.add(obs,
    action, [0], episode_start, value, log_prob)`` in ``get_action`` and ``buf.rewards[pos - 1] +=
    reward`` in ``update`` (pantheonrl/common/agents.py:112-214) -- for a whole batch, in
    PREALLOCATED ``[n_steps][...][n]`` device tensors whose write position is itself a device scalar.
    Every write is an ``index_copy_`` / ``index_add_`` on that scalar, so recording neither
    synchronises nor changes shape: it can sit inside a captured hipGraph (a learner's hook that runs
    host code per step cannot).  ``full()`` / ``steps()`` read the counter (one sync, when asked);
    ``reset()`` starts the next rollout.  Past ``n_steps`` the position wraps (a ring).

    ``fused=True``: the same tensors and counters, written by ``liboc_rollout.so``
    (include/oc_rollout.h) -- ONE launch per ``add``, one per ``add_reward`` (about a dozen and four
    torch launches otherwise), storing the same bits -- plus ``advantages`` / ``returns`` filled by
    ONE launch of ``compute_returns_and_advantage`` (the third buffer call of agents.py:127-131).

    ``state_window=W`` (a fused sink only, W dividing ``n_steps``): the sink also holds ``lstm_states``, float32
    ``[n_steps / W][2][64][n]`` -- room for a recurrent seat's (h, c) before the step of every W-th slot, which a
    ``FusedRecurrentPartner`` records there (include/oc_policy.h: ``oc_policy_window_snapshot``) and from which
    ``RecurrentPPOLearner`` unrolls windows of W steps.  ``None``: no such tensor, nothing changes."""

    def __init__(self, n_steps, n, rows, device="cuda", obs_dtype=torch.int32, fused=False, state_window=None):
        dev = torch.device(device)
        T = self.n_steps = int(n_steps)
        self.state_window = self.lstm_states = None
        if state_window is not None:
            W = int(state_window)
            if not fused:
                raise ValueError("state_window needs a RolloutSink(fused=True): the snapshot kernel reads the sink's "
                                 "position as a device word")
            if W < 1 or T % W:
                raise ValueError("state_window %d does not divide the sink's %d steps" % (W, T))
            self.state_window = W
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.obs = z((T, int(rows), n), obs_dtype)       # the viewer's [F][n] rows as they lie
        self.timestep = z((T, n), torch.float64)
        self.actions = z((T, 2, n), torch.int32)         # (move, comm)
        self.log_probs = z((T, n), torch.float32)
        self.values = z((T, n), torch.float32)
        self.rewards = z((T, n), torch.float64)
        self.episode_starts = z((T, n), torch.float32)
        self.dones = z((T, n), torch.int32)
        self.pos = z((1,), torch.int64)                  # next slot
        self.last = z((1,), torch.int64)                 # slot of the most recent add()
        self.count = z((1,), torch.int64)                # adds since reset()
        self.advantages = self.returns = self.ticket = None
        self.returns_ready = False                       # compute_returns_and_advantage ran since reset()
        self.fused = bool(fused)
        if self.fused:
            # one launch per add / add_reward / compute_returns_and_advantage (include/oc_rollout.h)
            if dev.type != "cuda":
                raise ValueError("the fused sink's kernels run on the GPU (device=%r); there is no CPU fallback" % (device,))
            if obs_dtype not in OBS_TYPE:
                raise ValueError("the fused sink stores int32, int8 or float32 rows (got %s)" % (obs_dtype,))
            self._L = _lib.load(lib="rollout")
            self.ticket = z((1,), torch.int32)           # the add kernel's workgroup ticket: 0 between calls
            self.advantages = z((T, n), torch.float32)
            self.returns = z((T, n), torch.float32)
            self._dev = dev.index if dev.index is not None else torch.cuda.current_device()
            self._buf = _lib.RolloutBuf(
                *[t.data_ptr() for t in (self.obs, self.timestep, self.actions, self.log_probs, self.values,
                                         self.episode_starts, self.rewards, self.dones, self.pos, self.last,
                                         self.count, self.ticket, self.advantages, self.returns)],
                n, T, int(rows), OBS_TYPE[obs_dtype])
            if self.state_window is not None:
                self.lstm_states = z((T // self.state_window, 2, 64, n), torch.float32)

    def _call(self, name, *args):
        """One entry point of liboc_rollout.so on the current torch stream of the sink's device."""
        _lib.call(self._L, name, self._dev, ctypes.byref(self._buf), *args)

    @staticmethod
    def _row(t, dtype, n):
        """t as the kernel reads it: `dtype`, contiguous, n elements (torch converts what is not)."""
        if t.dtype != dtype:
            t = t.to(dtype)
        t = t.reshape(-1)
        if t.numel() != n:
            raise ValueError("a row of %d elements where the sink holds %d envs" % (t.numel(), n))
        return t if t.is_contiguous() else t.contiguous()

    def add(self, rows, timestep, move, comm, log_prob, value, episode_start):
        if self.fused:
            n = self.obs.shape[2]
            if rows.dtype != self.obs.dtype or rows.shape != self.obs.shape[1:]:
                raise ValueError("rows %s %s where the sink holds %s %s" % (
                    rows.dtype, tuple(rows.shape), self.obs.dtype, tuple(self.obs.shape[1:])))
            # converted exactly as the torch path below converts them; what already lies as the kernel
            # reads it (the env's rows, its action rows, the partner's float32 rows) is passed as it is
            rows = rows if rows.is_contiguous() else rows.contiguous()
            keep = (rows, self._row(timestep, torch.float64, n), self._row(move, torch.int32, n),
                    self._row(comm, torch.int32, n), self._row(log_prob, torch.float32, n),
                    None if value is None else self._row(value, torch.float32, n),
                    self._row(episode_start, torch.float32, n))
            self._call("oc_rollout_add", *[None if t is None else t.data_ptr() for t in keep])
            return
        i = self.pos
        self.obs.index_copy_(0, i, rows.unsqueeze(0))
        self.timestep.index_copy_(0, i, timestep.unsqueeze(0))
        self.actions.index_copy_(0, i, torch.stack([move, comm]).to(torch.int32).unsqueeze(0))
        self.log_probs.index_copy_(0, i, log_prob.to(torch.float32).unsqueeze(0))
        if value is not None:
            self.values.index_copy_(0, i, value.reshape(1, -1).to(torch.float32))
        self.episode_starts.index_copy_(0, i, episode_start.to(torch.float32).unsqueeze(0))
        self.rewards.index_fill_(0, i, 0.0)              # buf.add(..., [0], ...): update() adds
        self.last.copy_(i)
        self.pos.add_(1).remainder_(self.n_steps)
        self.count.add_(1)

    def add_reward(self, rewards, dones):
        """``update(reward, done)`` of the step the most recent ``add`` belongs to."""
        if self.fused:
            n = self.obs.shape[2]
            keep = (self._row(rewards, torch.float64, n), self._row(dones, torch.int32, n))
            self._call("oc_rollout_add_reward", keep[0].data_ptr(), keep[1].data_ptr())
            return
        self.rewards.index_add_(0, self.last, rewards.to(torch.float64).unsqueeze(0))
        self.dones.index_copy_(0, self.last, dones.to(torch.int32).unsqueeze(0))

    def compute_returns_and_advantage(self, last_values, dones, gamma=0.99, gae_lambda=0.95):
        """stable-baselines3's ``RolloutBuffer.compute_returns_and_advantage`` over the recorded steps
        (what ``OnPolicyAgent.get_action`` calls on a full buffer before ``train()``, agents.py:127-131):
        ``last_values`` are the values of the observation after the newest step, ``dones`` whether
        that step ended its episode.  With L = min(count, n_steps), step k of L lives in slot
        (pos - L + k) mod n_steps; per env, in float32 and in this order (include/oc_rollout.h):

            delta = ((float)rewards[k] + (g * next_value) * next_non_terminal) - values[k]
            last  = delta + ((g_lambda * next_non_terminal) * last)
            advantages[k] = last;  returns[k] = last + values[k]

        Fills and returns ``(advantages, returns)``, float32 [n_steps][n]; slots that hold no step are
        left as they were.  ``fused=True``: ONE launch, no synchronisation.  Otherwise the loop in
        torch: a few launches per step and one read of the counters -- slow, and the same bits."""
        n = self.obs.shape[2]
        self.returns_ready = True
        if self.fused:
            keep = (self._row(last_values, torch.float32, n), self._row(dones, torch.float32, n))
            self._call("oc_rollout_gae", keep[0].data_ptr(), keep[1].data_ptr(),
                       ctypes.c_double(float(gamma)), ctypes.c_double(float(gae_lambda)))
            return self.advantages, self.returns
        if self.advantages is None:
            self.advantages = torch.zeros_like(self.values)
            self.returns = torch.zeros_like(self.values)
        T = self.n_steps
        g = float(np.float32(gamma))                                # exact in float32 from here on
        gl = float(np.float32(float(gamma) * float(gae_lambda)))    # the product in double, as SB3 forms it
        L, pos = min(self.steps(), T), int(self.pos.item())
        nv = last_values.reshape(-1).to(torch.float32)
        nnt = 1.0 - dones.reshape(-1).to(torch.float32)
        last = torch.zeros_like(nv)
        for k in range(L - 1, -1, -1):
            s = (pos - L + k) % T
            v = self.values[s]
            delta = (self.rewards[s].to(torch.float32) + (nv * g) * nnt) - v
            last = delta + ((nnt * gl) * last)
            self.advantages[s] = last
            self.returns[s] = last + v
            nv, nnt = v, 1.0 - self.episode_starts[s]
        return self.advantages, self.returns

    def steps(self):
        return int(self.count.item())

    def full(self):
        return self.steps() >= self.n_steps

    def reset(self):
        self.returns_ready = False
        self.pos.zero_()
        self.last.zero_()
        self.count.zero_()
        if self.ticket is not None:
            self.ticket.zero_()

    def get_state(self):
        st = self.pos.clone(), self.last.clone(), self.count.clone()
        return st if self.lstm_states is None else st + (self.lstm_states.clone(),)

    def set_state(self, st):
        self.pos.copy_(st[0])
        self.last.copy_(st[1])
        self.count.copy_(st[2])
        if self.lstm_states is not None:
            self.lstm_states.copy_(st[3])
