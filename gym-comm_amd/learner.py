"""``PPOLearner``: the PPO update of a ``FusedActorCriticPartner``'s ``MLPActorCritic`` as three
launches per minibatch (include/oc_policy.h: ``oc_policy_ppo_update``); ``RecurrentPPOLearner``: the update of a
``FusedRecurrentPartner``'s ``LSTMActorCritic`` over whole recorded sequences, six launches per minibatch
(``oc_policy_rppo_update``).  Both run a whole ``train()`` on device-side state as well (``shuffle="device"``,
``train_graph``: the train sequence of include/oc_policy.h), and the recurrent learner trains on WINDOWS of a rollout too,
from the states its seat recorded mid-rollout (``update_windows``, ``train_windows``, ``train_graph_windows``:
``oc_policy_window_gather`` in front of the same update) -- see ``vec_env`` for the overview."""
import ctypes

import torch

from . import _lib
from .batched import OBS_TYPE
from .partners import FusedActorCriticPartner, FusedRecurrentPartner, pack_lstm_bwd, pack_w2t

STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm",
         "adv_mean", "adv_std", "bad", "loss")
PARAMS = ("w1", "wt", "b1", "w2", "b2", "wv", "bv")        # the order of the flat gradient [P]
TRAIN_STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss")   # train_stats()
RECURRENT_PARAMS = ("wx", "wt", "b", "wh", "w2", "b2", "wv", "bv")   # the order of the recurrent learner's [P]


class _Learner:
    """What the two learners share: the checked master weights, Adam's state, the flat gradient with its views,
    the statistics, the device-side hyper-parameters, the scratch that regrows by retiring, the checks of
    a sink before ``train()``, and the train sequence's device state (include/oc_policy.h: ``oc_ppo_train``) with
    what reads and captures it: ``set_clip_range_vf`` / ``set_target_kl``, ``train_stats``, ``train_graph``'s body."""

    def _init_state(self, seat, names, P, lr, clip_range, ent_coef, vf_coef, max_grad_norm, betas, eps, max_groups):
        pol = seat.policy
        self.seat, self.policy = seat, pol
        self._L = seat._L
        self.F, self.C = seat.F, seat.C
        self._params = [getattr(pol, k) for k in names]
        for k, t in zip(names, self._params):
            if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("parameter %s: a contiguous float32 CUDA tensor (there is no CPU fallback)" % k)
            if t.device != seat.weight_device:
                raise ValueError("parameter %s lives on %s, the seat's packed weights on %s" % (k, t.device, seat.weight_device))
        dev = self.device = self._params[0].device
        self._dev = dev.index if dev.index is not None else torch.cuda.current_device()
        self.P = int(P)
        if self.P != sum(t.numel() for t in self._params):
            raise ValueError("the module has %d parameters, the kernel's layout %d" % (sum(t.numel() for t in self._params), P))
        z = self._zeros
        self.m, self.v, self.grad_flat = z(self.P), z(self.P), z(self.P)
        self.step = z(1, torch.int32)
        self.stats_t = z(len(STATS))
        self.hyper = torch.tensor([lr, clip_range], dtype=torch.float32, device=dev)
        self.grads, o = {}, 0
        for k, t in zip(names, self._params):
            self.grads[k] = self.grad_flat[o:o + t.numel()].view(t.shape)
            o += t.numel()
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        self.betas, self.eps, self.max_groups = (float(betas[0]), float(betas[1])), float(eps), int(max_groups)
        self._scratch, self._retired = None, []
        self._cfgs = {}
        self.lp_out = self.v_out = None          # set to float tensors to receive the forward (tests)

    def _init_train_state(self, clip_range_vf, target_kl):
        """The train sequence's device state (include/oc_policy.h: oc_ppo_train); 0 = off."""
        z, dev = self._zeros, self.device
        self.hyper_ext = torch.tensor([clip_range_vf or 0.0, target_kl or 0.0], dtype=torch.float32, device=dev)
        # (ctl and acc are views of one buffer: train_stats() fetches both with one copy)
        self._train_words = z(_lib.PPO_ACC["words"] + _lib.PPO_CTL["words"] // 2, torch.float64)
        self.acc = self._train_words[:_lib.PPO_ACC["words"]]
        self.ctl = self._train_words[_lib.PPO_ACC["words"]:].view(torch.int32)
        self._idx, self._trains = None, {}

    def _zeros(self, n, dt=torch.float32):
        return torch.zeros(n, dtype=dt, device=self.device)

    def _grow_scratch(self, need):
        if self._scratch is None or self._scratch.numel() < need:
            self._retired.append(self._scratch)           # a captured graph may still write to it
            self._scratch = torch.zeros(need, dtype=torch.float32, device=self.device)
            self._cfgs.clear()

    def _sink_tensors(self, sink, names):
        """The sink's tensors a cfg points at, checked; returns (tensors, T, n)."""
        for name in names:
            t = getattr(sink, name, None)
            if t is None or t.device != self.device or not t.is_contiguous():
                raise ValueError("the sink's %s: a contiguous tensor on %s (a fused sink has advantages / returns)"
                                 % (name, self.device))
        T, F, n = sink.obs.shape
        if F != self.F:
            raise ValueError("the policy was built for %d observation rows, the sink holds %d" % (self.F, F))
        if sink.obs.dtype not in OBS_TYPE:
            raise ValueError("the kernel reads int32, int8 or float32 rows (got %s)" % (sink.obs.dtype,))
        return tuple(getattr(sink, name) for name in names), T, n

    # ---- hyper-parameters read on the device ----
    def set_lr(self, lr):
        self.hyper[0] = float(lr)

    def set_clip_range(self, clip_range):
        self.hyper[1] = float(clip_range)

    def set_clip_range_vf(self, clip_range_vf):
        """Value clipping of the train sequence (``shuffle="device"``, ``train_graph``); None = off."""
        self.hyper_ext[0] = float(clip_range_vf or 0.0)

    def set_target_kl(self, target_kl):
        """The train sequence's early stop: no epoch after one whose mean approx_kl exceeds
        1.5 ``target_kl``; None = off."""
        self.hyper_ext[1] = float(target_kl or 0.0)

    def _check_outs(self, B):
        for t in (self.lp_out, self.v_out):
            if t is not None and (t.dtype != torch.float32 or t.numel() < B or not t.is_contiguous()):
                raise ValueError("lp_out / v_out: contiguous float32 tensors of at least B elements")

    def _check_trainable(self, sink, granule):
        """train()'s checks of the sink; returns the granule to use (1 if it does not divide the envs)."""
        if not getattr(sink, "fused", False):
            raise ValueError("train() needs a RolloutSink(fused=True): it holds advantages and returns")
        if not getattr(sink, "returns_ready", False):
            raise ValueError("train() needs the sink's advantages: call finish_rollout() "
                             "(compute_returns_and_advantage) first")
        if not sink.full():
            raise ValueError("train() needs a full sink (%d of %d steps recorded)" % (sink.steps(), sink.n_steps))
        n = sink.obs.shape[2]
        return 1 if granule > 1 and n % granule else int(granule)

    def stats(self):
        """The last minibatch's statistics as a dict: ONE synchronisation, and only when called."""
        return dict(zip(STATS, self.stats_t.cpu().tolist()))

    # ---- the train sequence: a whole train() on device-side state ----
    def _train_state(self, sink):
        tr = self._trains.get(id(sink))
        if tr is None:
            v = getattr(sink, "values", None)
            if v is None or v.device != self.device or v.dtype != torch.float32 or not v.is_contiguous() \
                    or v.shape != sink.advantages.shape:
                raise ValueError("the sink's values: a contiguous float32 [T][n] tensor on %s" % (self.device,))
            tr = _lib.PpoTrain(v.data_ptr(), self.hyper_ext.data_ptr(), self.ctl.data_ptr(), self.acc.data_ptr())
            tr._keep = (v,)
            self._trains[id(sink)] = tr
        return tr

    def _index_buffer(self, total):
        """The learner's own index buffer of at least ``total`` int32; regrows by retiring, as the scratch does."""
        if self._idx is None or self._idx.numel() < total:
            self._retired.append(self._idx)               # a captured graph may still write to it
            self._idx = torch.zeros(total, dtype=torch.int32, device=self.device)
        return self._idx

    def _capture(self, sink, sequence):
        """``train_graph``'s body: ``sequence(n_epochs)`` runs once eagerly for one epoch (every kernel is loaded,
        the index buffer and the scratch are sized), the learner's state is put back, and the capture of
        ``sequence(None)`` -- the caller's number of epochs -- follows."""
        with _lib.on_device(self._dev):
            state = self._train_tensors()
            saved = [t.clone() for t in state]
            sequence(1)
            torch.cuda.synchronize(self.device)
            with torch.no_grad():
                for t, s in zip(state, saved):
                    t.copy_(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sequence(None)
        return TrainGraph(self, sink, graph)

    def train_stats(self):
        """The reference's logged means over the updates APPLIED in the last train sequence -- policy_loss,
        value_loss, entropy_loss, approx_kl, clip_fraction, loss -- with ``updates``, ``epochs`` (completed)
        and ``stopped`` (by the KL rule).  ONE synchronisation, and only when called."""
        host = self._train_words.cpu()
        na = _lib.PPO_ACC["words"]
        acc, ctl = host[:na].tolist(), host[na:].view(torch.int32).tolist()
        if ctl[_lib.PPO_CTL["error"]]:
            raise _lib.OcError("the train sequence halted: a permutation walk reached its cap (include/oc_policy.h)")
        updates = ctl[_lib.PPO_CTL["updates"]]
        out = {k: (acc[_lib.PPO_ACC["sums"] + i] / updates if updates else float("nan"))
               for i, k in enumerate(TRAIN_STATS)}
        out.update(updates=updates, stopped=bool(ctl[_lib.PPO_CTL["stop"]]),
                   epochs=ctl[_lib.PPO_CTL["epochs"]] + (1 if acc[_lib.PPO_ACC["epoch_count"]] > 0 else 0))
        return out


class PPOLearner(_Learner):
    """What ``train()`` of the reference's PPO does per minibatch (pantheonrl/algos/modular/learn.py:
    222-334, stable-baselines3's, ``clip_range_vf=None``, no marginal regularisation) for the module
    of a ``FusedActorCriticPartner``: advantage normalisation, the clipped loss, its gradient, the
    norm clip, Adam, and the repack of the seat's fragment tensors -- all on the device, in place,
    without a synchronisation, capturable into a graph.  The learner owns Adam's ``m``, ``v`` and step
    counter, the scratch, the statistics and the flat gradient ``grad_flat`` (``grads[name]`` are views of it).
    ``lr`` and ``clip_range`` live in a device tensor (``hyper``): ``set_lr`` / ``set_clip_range`` are
    device writes, so a schedule needs no new capture.

    A whole ``train()`` can run on device-side state as well (``train(shuffle="device")``,
    ``train_graph``: include/oc_policy.h, the train sequence): the epoch's permutation, stable-baselines3's
    ``clip_range_vf``, the reference's ``target_kl`` stop and the logged means (``train_stats``) then
    need neither a torch op nor a synchronisation, and the sequence is one graph."""

    def __init__(self, seat, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 betas=(0.9, 0.999), eps=1e-5, max_groups=0, clip_range_vf=None, target_kl=None):
        if not isinstance(seat, FusedActorCriticPartner):
            raise TypeError("PPOLearner updates a gym_comm_amd.vec_env.FusedActorCriticPartner")
        plan = (ctypes.c_int32 * 4)()
        _lib.check(seat._L.oc_policy_ppo_plan(seat.F, seat.C, 2, 0, plan), "oc_policy_ppo_plan", seat._L)
        self._init_state(seat, PARAMS, plan[2], lr, clip_range, ent_coef, vf_coef, max_grad_norm, betas, eps, max_groups)
        self._init_train_state(clip_range_vf, target_kl)
        self._w2t = self._zeros(2 * 16 * 64)
        self.refresh()

    def refresh(self):
        """After the module's weights were changed from OUTSIDE (a checkpoint loaded, say): repack the
        seat's fragments (``seat.refresh()``) and the learner's transposed image, in place (a captured
        graph keeps the address).  ``update`` keeps both current itself."""
        self.seat.refresh()
        self._w2t.copy_(torch.from_numpy(pack_w2t(self._L, self.policy).reshape(-1)))

    # ---- one minibatch ----
    def plan(self, B):
        """(workgroups, tiles per wave, P, scratch floats) of a minibatch of B samples."""
        plan = (ctypes.c_int32 * 4)()
        _lib.check(self._L.oc_policy_ppo_plan(self.F, self.C, int(B), self.max_groups, plan), "oc_policy_ppo_plan", self._L)
        return tuple(int(v) for v in plan)

    def _cfg(self, sink, B):
        self._grow_scratch(max(self.plan(B)[3], 64 * (self.P + 8)))    # the default cap's worth at once: no regrowth
        key = (id(sink), self.max_groups, None if self.lp_out is None else self.lp_out.data_ptr(),
               None if self.v_out is None else self.v_out.data_ptr())
        cfg = self._cfgs.get(key)
        if cfg is None:
            keep, T, n = self._sink_tensors(sink, ("obs", "timestep", "actions", "log_probs", "advantages", "returns"))
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            cfg = _lib.PpoCfg(
                *[t.data_ptr() for t in keep], n, T, self.F, self.C, OBS_TYPE[sink.obs.dtype],
                *self.seat.weight_ptrs(), self._w2t.data_ptr(),
                *[t.data_ptr() for t in self._params],
                self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.grad_flat.data_ptr(),
                self._scratch.data_ptr(), self.stats_t.data_ptr(), self.hyper.data_ptr(),
                self.ent_coef, self.vf_coef, self.max_grad_norm, self.betas[0], self.betas[1], self.eps,
                self.max_groups, ptr(self.lp_out), ptr(self.v_out))
            cfg._keep = keep
            self._cfgs[key] = cfg
        return cfg

    def _run(self, name, sink, idx):
        if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous() or idx.device != self.device:
            raise ValueError("idx: a contiguous int32 [B] tensor on %s" % (self.device,))
        B = idx.numel()
        self._check_outs(B)
        _lib.call(self._L, name, self._dev, ctypes.byref(self._cfg(sink, B)), idx.data_ptr(), B)

    def update(self, sink, idx):
        """One minibatch: loss, gradient, clip, Adam, repack.  Three launches, no synchronisation."""
        self._run("oc_policy_ppo_update", sink, idx)

    def grad(self, sink, idx):
        """The clipped gradient (``grad_flat`` [P]; ``grads[name]`` are views of it, returned) and the
        statistics only: a caller with its own optimiser, and the tests."""
        self._run("oc_policy_ppo_grad", sink, idx)
        return self.grads

    # ---- epochs ----
    def minibatches(self, sink, batch_size, granule=32, generator=None):
        """A device permutation of the sink's T * n samples, cut into int32 index tensors of
        ``batch_size`` (the last one may be shorter; a remainder of one sample is dropped).
        ``granule=32`` shuffles tiles of 32 neighbouring envs of a slot -- the envs are independent, and a
        tile's rows load coalesced; ``granule=1`` is stable-baselines3's full shuffle.  The kernel treats
        both alike: every lane has its own index."""
        T, _, n = sink.obs.shape
        g = int(granule)
        if g < 1 or n % g:
            raise ValueError("granule %d does not divide the sink's %d envs" % (g, n))
        perm = torch.randperm(T * n // g, device=self.device, generator=generator)
        idx = (perm.unsqueeze(1) * g + torch.arange(g, device=self.device)).reshape(-1).to(torch.int32)
        return [b for b in idx.split(int(batch_size)) if b.numel() >= 2]

    def train(self, sink, n_epochs=10, batch_size=None, granule=32, generator=None, shuffle="torch", seed=0):
        """``n_epochs`` passes over a FULL fused sink whose ``compute_returns_and_advantage`` has run
        (``finish_rollout``).  ``batch_size=None``: the whole buffer as one minibatch.

        ``shuffle="torch"``: ``minibatches`` (torch.randperm, ``generator``) and one ``update`` each.
        ``shuffle="device"``: the train sequence of include/oc_policy.h, launched eagerly -- the
        permutation of (``seed``, the learner's device-side epoch counter) written into the learner's
        own index buffer, value clipping (``clip_range_vf``), the KL stop (``target_kl``) and the
        statistics ``train_stats()`` reports all on the device; the same launches ``train_graph`` captures."""
        granule = self._check_trainable(sink, granule)
        if shuffle == "device":
            return self._sequence(sink, int(n_epochs), batch_size, granule, seed)
        if shuffle != "torch":
            raise ValueError("shuffle: 'torch' or 'device' (got %r)" % (shuffle,))
        T, _, n = sink.obs.shape
        for _ in range(int(n_epochs)):
            for idx in self.minibatches(sink, batch_size or T * n, granule, generator):
                self.update(sink, idx)

    # ---- the train sequence: a whole train() on device-side state (the state and its readers: _Learner) ----
    def _sequence(self, sink, n_epochs, batch_size, granule, seed):
        """train_begin, then per epoch epoch_begin and one train_step per minibatch: a fixed, serial
        list of launches on the current stream -- no allocation after the first call for a sink's size,
        no synchronisation.  The minibatches are ``minibatches``' sizes, cut from the index buffer in order."""
        T, _, n = sink.obs.shape
        total = T * n
        bs = int(batch_size or total)
        if bs < 1:
            raise ValueError("batch_size must be positive")
        sizes = [min(bs, total - o) for o in range(0, total, bs)]
        cuts = [(o, b) for o, b in zip(range(0, total, bs), sizes) if b >= 2]
        self._check_outs(max(sizes))
        idx, tr, L, dev = self._index_buffer(total).data_ptr(), ctypes.byref(self._train_state(sink)), self._L, self._dev
        seed = int(seed) & 0xFFFFFFFF
        _lib.call(L, "oc_policy_ppo_train_begin", dev, tr)
        for _ in range(n_epochs):
            _lib.call(L, "oc_policy_ppo_epoch_begin", dev, tr, idx, total, granule, seed)
            for o, b in cuts:
                _lib.call(L, "oc_policy_ppo_train_step", dev, ctypes.byref(self._cfg(sink, b)), tr, idx + 4 * o, b)

    def _train_tensors(self):
        """Everything a train sequence writes that a later one reads."""
        return list(self._params) + [self.m, self.v, self.step, self._w2t, self.stats_t, self.grad_flat,
                                     self._train_words] + list(self.seat._w)

    def train_graph(self, sink, n_epochs, batch_size=None, granule=32, seed=0):
        """``train(shuffle="device")`` captured into ONE graph: a strictly serial stream of launches, no
        parallel branch.  The sequence runs once eagerly first (every kernel is loaded before the
        capture), the learner's state is put back, and the capture follows.  Returns an object whose
        ``replay()`` is one train(): the epoch counter lives on the device, so every replay shuffles anew,
        and ``set_lr`` / ``set_clip_range`` / ``set_clip_range_vf`` / ``set_target_kl`` act on the next replay."""
        granule = self._check_trainable(sink, granule)
        return self._capture(sink, lambda epochs: self._sequence(sink, int(epochs or n_epochs), batch_size, granule, seed))


class TrainGraph:
    """A captured train sequence (``PPOLearner.train_graph``, ``RecurrentPPOLearner.train_graph``): ``replay()``
    is one train()."""

    def __init__(self, learner, sink, graph):
        self.learner, self.sink, self.graph = learner, sink, graph

    def replay(self):
        self.graph.replay()


def env_cuts(n, T, envs_per_batch=None):
    """The recurrent learner's minibatches as (offset, E) into a permutation of n envs: chunks of ``envs_per_batch``
    envs in order (None: all of them), the last one shorter; one whose E T would be below 2 is dropped --
    ``RecurrentPPOLearner.minibatches``' sizes."""
    per = int(envs_per_batch or n)
    if per < 1:
        raise ValueError("envs_per_batch must be positive")
    return [(o, min(per, n - o)) for o in range(0, n, per) if min(per, n - o) * T >= 2]


def sequence_ids(n, T, W):
    """The ids of a rollout's windows as (window, env) -- include/oc_policy.h, "windows of a rollout": sequence
    s = k n + env is window k (slots k W .. k W + W - 1) of env ``env``; returns two int64 CPU tensors [n T / W]."""
    n, T, W = int(n), int(T), int(W)
    if W < 1 or T % W:
        raise ValueError("window %d does not divide the rollout's %d steps" % (W, T))
    s = torch.arange(n * (T // W))
    return s // n, s % n


def sequence_cuts(count, W, sequences_per_batch=None):
    """The windowed train()'s minibatches as (offset, E) into a permutation of ``count`` sequence ids: ``env_cuts``
    with a window's W steps per sequence."""
    return env_cuts(count, W, sequences_per_batch)


class _WindowBatch:
    """The learner's staging for a minibatch of windows (include/oc_policy.h: oc_window_batch): flat storage for up
    to ``cap`` sequences of W steps, which a minibatch of E <= cap sequences uses from its start, laid out as a sink
    of W slots and E envs; the start states ``h0`` / ``c0`` ([64][E]) and the constant ``envs`` = 0 .. cap - 1 whose
    first E elements the update is handed."""
    FLOATS = ("log_probs", "advantages", "returns", "episode_starts", "values")

    def __init__(self, W, F, cap, obs_dtype, device):
        z = lambda count, dt: torch.zeros(count, dtype=dt, device=device)  # noqa: E731
        self.W, self.F, self.cap, self.obs_dtype = W, F, cap, obs_dtype
        self.obs = z(W * F * cap, obs_dtype)
        self.timestep = z(W * cap, torch.float64)
        self.actions = z(W * 2 * cap, torch.int32)
        for name in self.FLOATS:
            setattr(self, name, z(W * cap, torch.float32))
        self.h0, self.c0 = z(64 * cap, torch.float32), z(64 * cap, torch.float32)
        self.envs = torch.arange(cap, dtype=torch.int32, device=device)
        self.c_struct = _lib.WindowBatch(*[t.data_ptr() for t in self.tensors()])

    def tensors(self):
        """The ten tensors in oc_window_batch's order."""
        return [self.obs, self.timestep, self.actions] + [getattr(self, k) for k in self.FLOATS] + [self.h0, self.c0]

    def fits(self, W, F, E, obs_dtype):
        return (self.W, self.F, self.obs_dtype) == (W, F, obs_dtype) and E <= self.cap

    def view(self, name, E):
        """Tensor ``name`` as a minibatch of E sequences sees it: [W][F][E], [W][2][E], [W][E] or [64][E]."""
        W, F = self.W, self.F
        shape = {"obs": (W, F, E), "actions": (W, 2, E), "h0": (64, E), "c0": (64, E)}.get(name, (W, E))
        count = 1
        for d in shape:
            count *= d
        return getattr(self, name)[:count].view(shape)


class RecurrentPPOLearner(_Learner):
    """The minibatch update of a ``FusedRecurrentPartner``'s ``LSTMActorCritic`` (include/oc_policy.h:
    ``oc_policy_rppo_update``): advantage normalisation, the forward over whole recorded sequences from the
    seat's ``h0`` / ``c0`` (``seat.begin_rollout()``), the clipped loss, backpropagation through time, the norm
    clip, Adam and the repack of the seat's three images -- six launches on the device, in place, without a
    synchronisation, capturable.  A minibatch is a set of ENVS (int32 ``envs`` [E], repeats allowed): every env
    brings its whole sequence of T steps, B = E T.  The learner owns what ``PPOLearner`` owns, and ``_bwd``, the
    backward's image of Wh and [W2; wv] transposed.  ``lp_out`` / ``v_out`` (float32 [T][E], tests) receive the
    forward.

    A whole ``train()`` can run on device-side state, as ``PPOLearner``'s does (``train(shuffle="device")``,
    ``train_graph``; include/oc_policy.h, last section: ``oc_policy_recurrent_train_step``): the epoch's
    permutation of the ENVS, stable-baselines3's ``clip_range_vf``, the ``target_kl`` stop and the logged means
    (``train_stats``) then need neither a torch op nor a synchronisation, and the sequence is one graph.  The KL
    rule is the reference's modular learner's, at the END of an epoch on the mean of ``approx_kl`` -- not
    sb3_contrib ``RecurrentPPO``'s break in mid-epoch.  ``set_lr`` / ``set_clip_range`` / ``set_clip_range_vf`` /
    ``set_target_kl`` are device writes: they act on the next replay.

    Windows (include/oc_policy.h, "windows of a rollout").  On a ``RolloutSink(..., state_window=W)`` whose seat
    recorded its state where every window begins, a minibatch can be a set of WINDOWS of W steps instead: int32
    ``seqs`` [E] of sequence ids (``sequence_ids``), each unrolled from its recorded state, which is a constant in
    the gradient (truncated backpropagation through time).  ``update_windows`` / ``grad_windows`` gather the
    minibatch into the learner's own window batch (one launch) and run the unchanged update on it as on a sink of
    W slots and E envs: seven launches.  ``train_windows`` / ``train_graph_windows`` are ``train`` / ``train_graph``
    over sequence ids.  Not here: windows that do not divide the rollout, a state recorded at every step,
    sb3_contrib's exact contiguous-chunk minibatches, the marginal-regularisation term."""

    def __init__(self, seat, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 betas=(0.9, 0.999), eps=1e-5, max_groups=0, clip_range_vf=None, target_kl=None):
        if not isinstance(seat, FusedRecurrentPartner):
            raise TypeError("RecurrentPPOLearner updates a gym_comm_amd.vec_env.FusedRecurrentPartner")
        plan = (ctypes.c_int64 * 8)()
        _lib.check(seat._L.oc_policy_rppo_plan(seat.F, seat.C, 1, 2, 0, plan), "oc_policy_rppo_plan", seat._L)
        self._init_state(seat, RECURRENT_PARAMS, plan[3], lr, clip_range, ent_coef, vf_coef, max_grad_norm, betas, eps,
                         max_groups)
        self._init_train_state(clip_range_vf, target_kl)
        self._bwd = self._zeros(self._L.oc_policy_rppo_pack_bwd_elems())
        self._wbatch, self._wsrcs = None, {}          # the window batch (allocated by the first windowed call)
        self.refresh()

    def refresh(self):
        """After the module's weights were changed from OUTSIDE: repack the seat's images (``seat.refresh()``)
        and the learner's backward image, in place.  ``update`` keeps them current itself."""
        self.seat.refresh()
        self._bwd.copy_(torch.from_numpy(pack_lstm_bwd(self._L, self.policy)))

    def plan(self, E, T):
        """(forward / backward workgroups, weight-gradient workgroups, (t, tile) pairs per such workgroup, P,
        scratch floats, reduction workgroups, launches, scratch floats per sample) of E sequences of T steps."""
        plan = (ctypes.c_int64 * 8)()
        _lib.check(self._L.oc_policy_rppo_plan(self.F, self.C, int(T), int(E), self.max_groups, plan),
                   "oc_policy_rppo_plan", self._L)
        return tuple(int(v) for v in plan)

    def _build_cfg(self, rollout_ptrs, h0, c0, n, T, obs_type):
        """An oc_rppo_cfg over the seven rollout tensors at ``rollout_ptrs`` and the start state (h0, c0)."""
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return _lib.RppoCfg(
            *rollout_ptrs, h0.data_ptr(), c0.data_ptr(), n, T, self.F, self.C,
            obs_type, *self.seat.weight_ptrs(), self._bwd.data_ptr(),
            *[t.data_ptr() for t in self._params],
            self.m.data_ptr(), self.v.data_ptr(), self.step.data_ptr(), self.grad_flat.data_ptr(),
            self._scratch.data_ptr(), self.stats_t.data_ptr(), self.hyper.data_ptr(),
            self.ent_coef, self.vf_coef, self.max_grad_norm, self.betas[0], self.betas[1], self.eps,
            self.max_groups, ptr(self.lp_out), ptr(self.v_out))

    def _cfg(self, sink, E):
        T = sink.obs.shape[0]
        self._grow_scratch(self.plan(E, T)[4])
        seat = self.seat
        key = (id(sink), self.max_groups, None if self.lp_out is None else self.lp_out.data_ptr(),
               None if self.v_out is None else self.v_out.data_ptr(), seat.h0.data_ptr())
        cfg = self._cfgs.get(key)
        if cfg is None:
            keep, T, n = self._sink_tensors(sink, ("obs", "timestep", "actions", "log_probs", "advantages", "returns",
                                                   "episode_starts"))
            if seat.h0 is None or tuple(seat.h0.shape) != (64, n):
                raise ValueError("the seat holds no start state for %d envs: call seat.begin_rollout() before the rollout" % n)
            cfg = self._build_cfg([t.data_ptr() for t in keep], seat.h0, seat.c0, n, T, OBS_TYPE[sink.obs.dtype])
            cfg._keep = keep + (seat.h0, seat.c0)
            self._cfgs[key] = cfg
        return cfg

    def _run(self, name, sink, envs):
        if envs.dtype != torch.int32 or envs.dim() != 1 or not envs.is_contiguous() or envs.device != self.device:
            raise ValueError("envs: a contiguous int32 [E] tensor on %s" % (self.device,))
        if self.seat.h0 is None:
            raise ValueError("the seat holds no start state: call seat.begin_rollout() before the rollout")
        E = envs.numel()
        self._check_outs(E * sink.obs.shape[0])
        _lib.call(self._L, name, self._dev, ctypes.byref(self._cfg(sink, E)), envs.data_ptr(), E)

    def update(self, sink, envs):
        """One minibatch of whole sequences: loss, BPTT, clip, Adam, repack.  Six launches, no synchronisation.
        The sink must be full with its slots in chronological order (``train`` checks it; here it is the
        caller's duty)."""
        self._run("oc_policy_rppo_update", sink, envs)

    def grad(self, sink, envs):
        """The clipped gradient (``grad_flat`` [P]; ``grads[name]`` are views of it, returned) and the
        statistics only."""
        self._run("oc_policy_rppo_grad", sink, envs)
        return self.grads

    def minibatches(self, sink, envs_per_batch, granule=32, generator=None):
        """A device permutation (``torch.randperm``) of the sink's envs, cut into int32 tensors of
        ``envs_per_batch``; ``granule=32`` shuffles tiles of 32 neighbouring envs, whose rows load coalesced.
        A last batch whose E T would be 1 is dropped."""
        T, _, n = sink.obs.shape
        g = int(granule)
        if g < 1 or n % g:
            raise ValueError("granule %d does not divide the sink's %d envs" % (g, n))
        perm = torch.randperm(n // g, device=self.device, generator=generator)
        envs = (perm.unsqueeze(1) * g + torch.arange(g, device=self.device)).reshape(-1).to(torch.int32)
        return [b for b in envs.split(int(envs_per_batch)) if b.numel() * T >= 2]

    def _check_chronological(self, sink, granule):
        """train()'s checks of the sink -- full, advantages ready, slots in chronological order (ONE
        synchronisation: ``pos``); returns the granule to use."""
        granule = self._check_trainable(sink, granule)
        if sink.steps() != sink.n_steps or int(sink.pos.item()) != 0:
            raise ValueError("train() needs the sink's slots in chronological order: exactly %d steps since "
                             "begin_rollout() (count %d, pos %d)" % (sink.n_steps, sink.steps(), int(sink.pos.item())))
        return granule

    def train(self, sink, n_epochs=10, envs_per_batch=None, granule=32, generator=None, shuffle="torch", seed=0):
        """``n_epochs`` passes over a FULL fused sink whose ``finish_rollout`` has run and whose slots are in
        chronological order (``count == n_steps``, ``pos == 0``: ``seat.begin_rollout()``, then exactly
        ``n_steps`` steps).  ``envs_per_batch=None``: every env in one minibatch.

        ``shuffle="torch"``: ``minibatches`` (torch.randperm, ``generator``) and one ``update`` each.
        ``shuffle="device"``: the train sequence of include/oc_policy.h, launched eagerly -- the permutation of
        the envs from (``seed``, the learner's device-side epoch counter) written into the learner's own index
        buffer, value clipping (``clip_range_vf``), the KL stop (``target_kl``) and the statistics
        ``train_stats()`` reports all on the device; the same launches ``train_graph`` captures."""
        if shuffle not in ("torch", "device"):
            raise ValueError("shuffle: 'torch' or 'device' (got %r)" % (shuffle,))
        granule = self._check_chronological(sink, granule)
        if shuffle == "device":
            return self._sequence(sink, int(n_epochs), envs_per_batch, granule, seed)
        n = sink.obs.shape[2]
        for _ in range(int(n_epochs)):
            for envs in self.minibatches(sink, envs_per_batch or n, granule, generator):
                self.update(sink, envs)

    # ---- the train sequence: a whole train() on device-side state (the state and its readers: _Learner) ----
    def _sequence(self, sink, n_epochs, envs_per_batch, granule, seed):
        """train_begin, then per epoch epoch_begin over the n envs and one recurrent train_step per cut of the
        index buffer (``env_cuts``): a fixed, serial list of launches on the current stream.  The scratch is sized
        once, for the largest cut, before the first launch; no allocation after the first call for a sink's
        size, no synchronisation."""
        T, _, n = sink.obs.shape
        if self.seat.h0 is None:
            raise ValueError("the seat holds no start state: call seat.begin_rollout() before the rollout")
        cuts = env_cuts(n, T, envs_per_batch)
        if not cuts:
            raise ValueError("no minibatch of at least 2 samples (%d envs x %d steps)" % (n, T))
        largest = max(E for _, E in cuts)
        self._grow_scratch(self.plan(largest, T)[4])
        self._check_outs(largest * T)
        idx, tr, L, dev = self._index_buffer(n).data_ptr(), ctypes.byref(self._train_state(sink)), self._L, self._dev
        cfg = ctypes.byref(self._cfg(sink, largest))
        seed = int(seed) & 0xFFFFFFFF
        _lib.call(L, "oc_policy_ppo_train_begin", dev, tr)
        for _ in range(n_epochs):
            _lib.call(L, "oc_policy_ppo_epoch_begin", dev, tr, idx, n, granule, seed)
            for o, E in cuts:
                _lib.call(L, "oc_policy_recurrent_train_step", dev, cfg, tr, idx + 4 * o, E)

    def _train_tensors(self):
        """Everything a train sequence writes that a later one reads (``seat.h0`` / ``c0`` are read only, and
        ``begin_rollout()`` writes them in place: a captured graph's addresses stay good)."""
        return list(self._params) + [self.m, self.v, self.step, self._bwd, self.stats_t, self.grad_flat,
                                     self._train_words] + list(self.seat._w)

    def train_graph(self, sink, n_epochs, envs_per_batch=None, granule=32, seed=0):
        """``train(shuffle="device")`` captured into ONE graph: a strictly serial stream of launches.  ``train()``'s
        host-side checks of the sink -- full, advantages ready, chronological order -- are made HERE, before the
        capture, and synchronise once; a replay cannot make them: the caller must replay only on a full,
        chronological, finished sink (``seat.begin_rollout()``, exactly ``n_steps`` steps, ``finish_rollout()``).
        The sequence runs once eagerly first, the learner's state is put back, and the capture follows.  Returns a
        ``TrainGraph`` whose ``replay()`` is one train(): the epoch counter lives on the device, so every replay
        shuffles anew, and ``set_lr`` / ``set_clip_range`` / ``set_clip_range_vf`` / ``set_target_kl`` act on the
        next replay."""
        granule = self._check_chronological(sink, granule)
        return self._capture(sink, lambda epochs: self._sequence(sink, int(epochs or n_epochs), envs_per_batch, granule, seed))

    # ---- windows: minibatches of W-step stretches from the states the seat recorded mid-rollout ----
    def sequences(self, sink):
        """How many windows the sink's rollout holds: ``n * n_steps // state_window``."""
        W = self._window(sink)
        T, _, n = sink.obs.shape
        return n * T // W

    @staticmethod
    def _window(sink):
        W = getattr(sink, "state_window", None)
        if W is None:
            raise ValueError("windows need a RolloutSink(..., state_window=W) whose seat recorded its states")
        return int(W)

    def _window_src(self, sink):
        """The sink as the gather reads it (oc_window_src), checked once per sink."""
        src = self._wsrcs.get(id(sink))
        if src is None:
            W = self._window(sink)
            keep, T, n = self._sink_tensors(sink, ("obs", "timestep", "actions", "log_probs", "advantages", "returns",
                                                   "episode_starts", "values", "lstm_states"))
            if tuple(sink.lstm_states.shape) != (T // W, 2, 64, n) or sink.lstm_states.dtype != torch.float32:
                raise ValueError("the sink's lstm_states: float32 [%d][2][64][%d]" % (T // W, n))
            src = _lib.WindowSrc(*[t.data_ptr() for t in keep], n, T, W, self.F, OBS_TYPE[sink.obs.dtype])
            src._keep = keep
            self._wsrcs[id(sink)] = src
        return src

    def _window_batch(self, sink, E):
        """The learner's own window batch with room for E sequences of the sink's windows; regrows by retiring, as
        the scratch and the index buffer do (a captured graph may still write to the old one)."""
        W, b = self._window(sink), self._wbatch
        if b is None or not b.fits(W, self.F, E, sink.obs.dtype):
            self._retired.append(b)
            b = self._wbatch = _WindowBatch(W, self.F, max(E, b.cap if b is not None else 0), sink.obs.dtype, self.device)
        return b

    def _batch_cfg(self, batch, E):
        """The cfg that shows the update E gathered sequences as a full sink of W slots and E envs."""
        self._grow_scratch(self.plan(E, batch.W)[4])
        key = (id(batch), E, self.max_groups, None if self.lp_out is None else self.lp_out.data_ptr(),
               None if self.v_out is None else self.v_out.data_ptr())
        cfg = self._cfgs.get(key)
        if cfg is None:
            keep = batch.tensors()
            cfg = self._build_cfg([t.data_ptr() for t in keep[:3]] + [getattr(batch, k).data_ptr() for k in
                                  ("log_probs", "advantages", "returns", "episode_starts")],
                                  batch.h0, batch.c0, E, batch.W, OBS_TYPE[batch.obs_dtype])
            cfg._keep = tuple(keep)
            self._cfgs[key] = cfg
        return cfg

    def _gather(self, sink, batch, seqs_ptr, E):
        _lib.call(self._L, "oc_policy_window_gather", self._dev, ctypes.byref(self._window_src(sink)),
                  ctypes.byref(batch.c_struct), seqs_ptr, E)

    def _run_windows(self, name, sink, seqs):
        if seqs.dtype != torch.int32 or seqs.dim() != 1 or not seqs.is_contiguous() or seqs.device != self.device:
            raise ValueError("seqs: a contiguous int32 [E] tensor on %s" % (self.device,))
        E = seqs.numel()
        batch = self._window_batch(sink, E)
        self._check_outs(E * batch.W)
        self._gather(sink, batch, seqs.data_ptr(), E)
        _lib.call(self._L, name, self._dev, ctypes.byref(self._batch_cfg(batch, E)), batch.envs.data_ptr(), E)

    def update_windows(self, sink, seqs):
        """One minibatch of WINDOWS: int32 ``seqs`` [E] of sequence ids (``sequence_ids``; any order, repeats
        allowed), each window unrolled from the state recorded where it begins.  One gather into the learner's
        window batch, then ``update``'s six launches on it: seven launches, no synchronisation.  ``lp_out`` /
        ``v_out`` receive float [W][E].  The sink must be full and chronological (``train_windows`` checks it)."""
        self._run_windows("oc_policy_rppo_update", sink, seqs)

    def grad_windows(self, sink, seqs):
        """The clipped gradient and the statistics of a minibatch of windows only (``grad``'s counterpart)."""
        self._run_windows("oc_policy_rppo_grad", sink, seqs)
        return self.grads

    def minibatches_windows(self, sink, sequences_per_batch, granule=32, generator=None):
        """A device permutation (``torch.randperm``) of the sink's sequence ids, cut into int32 tensors of
        ``sequences_per_batch``; ``granule`` must divide the envs, so that a tile of ``granule`` ids stays inside one
        window and its rows load coalesced."""
        W, count = self._window(sink), self.sequences(sink)
        n, g = sink.obs.shape[2], int(granule)
        if g < 1 or n % g:
            raise ValueError("granule %d does not divide the sink's %d envs" % (g, n))
        perm = torch.randperm(count // g, device=self.device, generator=generator)
        seqs = (perm.unsqueeze(1) * g + torch.arange(g, device=self.device)).reshape(-1).to(torch.int32)
        return [b for b in seqs.split(int(sequences_per_batch)) if b.numel() * W >= 2]

    def train_windows(self, sink, n_epochs=10, sequences_per_batch=None, granule=32, generator=None, shuffle="torch",
                      seed=0):
        """``train`` over WINDOWS of ``sink.state_window`` steps: the same checks of the sink, the same two shuffles,
        the same train sequence -- over the n T / W sequence ids instead of the n envs, with one gather in front of
        every minibatch.  ``sequences_per_batch=None``: every window in one minibatch.  With ``shuffle="device"``,
        ``clip_range_vf`` clips about the recorded values of the gathered samples, and the KL rule, ``train_stats()``
        and the setters are ``train``'s."""
        if shuffle not in ("torch", "device"):
            raise ValueError("shuffle: 'torch' or 'device' (got %r)" % (shuffle,))
        self._window(sink)
        granule = self._check_chronological(sink, granule)
        if shuffle == "device":
            return self._sequence_windows(sink, int(n_epochs), sequences_per_batch, granule, seed)
        for _ in range(int(n_epochs)):
            for seqs in self.minibatches_windows(sink, sequences_per_batch or self.sequences(sink), granule, generator):
                self.update_windows(sink, seqs)

    def _sequence_windows(self, sink, n_epochs, sequences_per_batch, granule, seed):
        """``_sequence`` over sequence ids: epoch_begin with count = n T / W, and per cut of the index buffer one
        gather and one recurrent train_step on the window batch.  The gather is not held back by a halted sequence:
        it writes the learner's staging only."""
        W, count = self._window(sink), self.sequences(sink)
        cuts = sequence_cuts(count, W, sequences_per_batch)
        if not cuts:
            raise ValueError("no minibatch of at least 2 samples (%d windows of %d steps)" % (count, W))
        largest = max(E for _, E in cuts)
        self._grow_scratch(self.plan(largest, W)[4])
        self._check_outs(largest * W)
        batch = self._window_batch(sink, largest)
        tr = self._trains.get(id(batch))
        if tr is None:
            tr = self._trains[id(batch)] = _lib.PpoTrain(batch.values.data_ptr(), self.hyper_ext.data_ptr(),
                                                         self.ctl.data_ptr(), self.acc.data_ptr())
            tr._keep = (batch,)
        idx, L, dev = self._index_buffer(count).data_ptr(), self._L, self._dev
        cfgs = {E: ctypes.byref(self._batch_cfg(batch, E)) for E in sorted({E for _, E in cuts}, reverse=True)}
        envs, seed = batch.envs.data_ptr(), int(seed) & 0xFFFFFFFF
        _lib.call(L, "oc_policy_ppo_train_begin", dev, ctypes.byref(tr))
        for _ in range(n_epochs):
            _lib.call(L, "oc_policy_ppo_epoch_begin", dev, ctypes.byref(tr), idx, count, granule, seed)
            for o, E in cuts:
                self._gather(sink, batch, idx + 4 * o, E)
                _lib.call(L, "oc_policy_recurrent_train_step", dev, cfgs[E], ctypes.byref(tr), envs, E)

    def train_graph_windows(self, sink, n_epochs, sequences_per_batch=None, granule=32, seed=0):
        """``train_windows(shuffle="device")`` captured into ONE graph, as ``train_graph`` captures ``train``: the
        checks of the sink are made here, before the capture; every replay shuffles anew."""
        self._window(sink)
        granule = self._check_chronological(sink, granule)
        return self._capture(sink, lambda epochs: self._sequence_windows(sink, int(epochs or n_epochs),
                                                                         sequences_per_batch, granule, seed))
