"""The numpy boundary of ``OvercookedVecEnv`` (see ``vec_env`` for the overview): how a step's arrays
cross PCIe.  ``pack_plan`` says where every observation row, reward, done flag and episode statistic
lies in one packed step (include/oc_hostio.h); a TRANSPORT moves that packed step to the host.  The two
transports have one contract --

    observe()        the ego's observation arrays of the current state (what ``reset()`` returns)
    start(actions)   begin a step from host actions [n, 2]
    finish()         end it: (obs dict, rewards float32 [n], done int32 [n], (returns, lengths) or None)
    close()          let a started step end

``HostCopy``: staged copies in and out and a blocking wait, all of it in ``finish``.  ``HostMapped``: the
kernels read the actions from host-mapped memory and write the packed step into it; ``start`` issues
everything, ``finish`` polls an event.  A transport is built on the env's first numpy call: tensor-only
users allocate no pinned or mapped memory."""
import collections
import ctypes
import time

import numpy as np
import torch

from . import _lib
from .batched import OBS_TYPE

# dtype each key has after SB3 copies it into a buffer of the declared space
# (gym_comm/envs/overcooked_env.py:41-85: Box float32 / Box int64 / MultiBinary int8)
SPACE_DTYPE = {
    "timestep": np.float32, "object_encodings_x": np.int64, "object_encodings_y": np.int64,
    "state_encodings": np.int8, "is_hidden": np.int8, "completed_subtasks": np.int8,
    "agent1_location": np.float32, "agent2_location": np.float32, "agent_is_holding": np.int8,
    "agent1_comm": np.int8, "agent2_comm": np.int8,
}

# words: int32 [F], row r -> (block << 16) | column; width: columns of the int64 / float32 / int8 block;
# cols: key -> (block, lo, hi); off: byte ranges of the packed step's parts; total: its bytes
PackPlan = collections.namedtuple("PackPlan", "words width cols off total stats")
PackOffsets = collections.namedtuple("PackOffsets", "b64 ret b32 ts rew done len b8")     # in this order


def pack_plan(layout, F, n, stats):
    """The pack plan of a step of ``n`` envs (include/oc_hostio.h): which observation row -- ``layout`` is
    ``obs_layout(S, C)``, ``F`` its rows -- goes to which column of which dtype block (int64 / float32 /
    int8 as the declared spaces), and where the blocks, timestep, reward, done flags and -- ``stats`` --
    episode return / length lie in the packed bytes.  Pure host code."""
    block_of = {np.dtype(np.int64): 0, np.dtype(np.float32): 1, np.dtype(np.int8): 2}
    width, words, cols = [0, 0, 0], np.zeros(F, np.int32), {}
    for k, (lo, hi) in layout.items():
        blk = block_of[np.dtype(SPACE_DTYPE[k])]
        cols[k] = (blk, width[blk], width[blk] + hi - lo)
        for r in range(lo, hi):
            words[r] = (blk << 16) | width[blk]
            width[blk] += 1
    sizes = (n * width[0] * 8, n * 8 if stats else 0, n * width[1] * 4, n * 4, n * 4, n * 4, n * 4 if stats else 0,
             n * width[2])
    ends = np.cumsum(sizes).tolist()
    off = PackOffsets(*zip([0] + ends[:-1], ends))
    return PackPlan(words, tuple(width), cols, off, ends[-1], bool(stats))


class MappedBuffer:
    """``nbytes`` of pinned host memory that kernels read and write in place (include/oc_hostio.h:
    ``oc_hostio_alloc``): ``dev`` is its address for kernels, ``view()`` a uint8 array over it for
    the host.  The object is the ``base`` of that array and so of every array cut from it: the
    memory is freed when the last of them and the last other reference to the object are gone.
    Nothing here waits for a kernel that may still be writing it (an env dropped between
    ``step_async`` and ``step_wait``): ``hipHostFree`` synchronises the device before it releases
    the memory, and that is what this relies on."""

    def __init__(self, L, dev_index, nbytes):
        host, dev = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.call(L, "oc_hostio_alloc", dev_index, int(nbytes), ctypes.byref(host), ctypes.byref(dev), stream=False)
        self._L, self.host, self.dev, self.nbytes = L, host.value, dev.value, int(nbytes)

    @property
    def __array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.host, False), "version": 3}

    def view(self):
        return np.asarray(self)

    def __del__(self):
        host, self.host = getattr(self, "host", None), None
        if host:
            try:
                self._L.oc_hostio_free(host)
            except Exception:                   # interpreter shutdown
                pass


class _Transport:
    """What the two transports share: the plan, the pack launch and the views of a packed step.
    ``venv``: the env (a weak proxy: the env owns its transport); ``reuse``: False = every step returns
    fresh arrays (a host copy out of the buffer); True = the arrays are views of two alternating
    buffers, valid until the step after next (what a rollout collector that copies them on arrival needs)."""
    act = None          # the actions' MappedBuffer: HostMapped, once the single-launch path has been taken
    _act_pinned = None  # the actions' pinned staging buffer, once a step has gone the other way

    def __init__(self, venv, reuse=False):
        b = venv._b
        self.venv, self.n, self.reuse, self.flip = venv, venv.num_envs, bool(reuse), 0
        self.L = L = _lib.load(lib="hostio")
        self.plan = p = pack_plan(b._layout, b.F, self.n, b.ep_return is not None)
        assert p.total == L.oc_pack_host_bytes(*p.width, 1, int(p.stats), 1, int(p.stats), self.n)
        self.nbytes = max(p.total, 1)
        self._words = torch.from_numpy(p.words).to(b.device)
        dp = lambda t: None if t is None else t.data_ptr()
        # (the batch's tensors are views of one arena for its whole life: their addresses are taken once)
        self._pack_args = (b._dev_index, b.obs[0].data_ptr(), OBS_TYPE[b.obs.dtype], b.F, self._words.data_ptr(),
                           *p.width, b.timestep.data_ptr(), b.shaped_reward.data_ptr(), dp(b.ep_return),
                           b.done.data_ptr(), dp(b.ep_length))

    def pack(self, name, out):
        """ONE launch of ``oc_pack_host`` / ``oc_pack_host_tiled`` (``name``): the ego viewer's [F][n] rows
        gathered by target dtype, transposed and converted; float32 timestep and reward, done flags,
        episode return / length -- into the bytes at device address ``out``."""
        _lib.call(self.L, name, *self._pack_args, out, self.n)

    def views(self, host):
        """(obs dict, rewards, done int32, episode stats) as views of one packed step ``host`` (uint8)."""
        n, p = self.n, self.plan
        view = lambda rng, dt, shape: host[rng[0]:rng[1]].view(dt).reshape(shape)
        blocks = (view(p.off.b64, np.int64, (n, p.width[0])), view(p.off.b32, np.float32, (n, p.width[1])),
                  view(p.off.b8, np.int8, (n, p.width[2])))
        obs = {k: blocks[blk][:, lo:hi] for k, (blk, lo, hi) in p.cols.items()}
        obs["timestep"] = view(p.off.ts, np.float32, (n, 1))
        stats = (view(p.off.ret, np.float64, (n,)), view(p.off.len, np.int32, (n,))) if p.stats else None
        return obs, view(p.off.rew, np.float32, (n,)), view(p.off.done, np.int32, (n,)), stats

    def staged(self, actions):
        """Host actions -> pinned staging -> the device pairs the kernel consumes as they lie."""
        if self._act_pinned is None:
            self._act_pinned = torch.empty((self.n, 2), dtype=torch.int32, pin_memory=True)
        np.copyto(self._act_pinned.numpy(), actions.reshape(self.n, 2), casting="unsafe")
        ego_pairs = self.venv._staged_pairs()
        ego_pairs.copy_(self._act_pinned, non_blocking=True)
        return ego_pairs

    def close(self):
        pass


class HostCopy(_Transport):
    """One pack launch into a device buffer, ONE device->host copy into pinned memory, a blocking
    wait, and (without ``reuse``) a host copy out of it; the actions go through a pinned staging
    buffer.  ``start`` only remembers the actions: the step runs in ``finish``."""

    def __init__(self, venv, reuse=False):
        super().__init__(venv, reuse)
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=venv._b.device)
        self.pinned = [torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2 if reuse else 1)]
        self._pending = None

    def observe(self):
        return self._fetch()[0]

    def start(self, actions):
        self._pending = np.asarray(actions)

    def finish(self):
        self.venv.step_tensors(self.staged(self._pending))
        return self._fetch()

    def _fetch(self):
        self.pack("oc_pack_host", self.dev.data_ptr())
        self.flip ^= 1
        pinned = self.pinned[self.flip if self.reuse else 0]
        pinned.copy_(self.dev, non_blocking=True)
        torch.cuda.current_stream(self.dev.device).synchronize()
        return self.views(pinned.numpy() if self.reuse else pinned.numpy().copy())


class HostMapped(_Transport):
    """The step kernel reads the actions from host-mapped memory (on the single-launch path; staged
    otherwise), ``oc_pack_host_tiled`` writes the packed step into one of two alternating host-mapped
    buffers, an event behind it ends the step: ``start`` issues all of that, ``finish`` polls the
    event (a blocked wait on this runtime can return tens of milliseconds late)."""
    timeout = 30.0

    def __init__(self, venv, reuse=False):
        super().__init__(venv, reuse)
        dev = venv._b._dev_index
        self.bufs = [MappedBuffer(self.L, dev, self.nbytes) for _ in range(2)]
        self.event = torch.cuda.Event()
        self._cut = [None, None]        # reuse: the views of each buffer, cut once
        self._act_np = None
        self.inflight = False           # a step was started and not finished

    def observe(self):
        self.close()
        self._pack()
        return self._wait()[0]

    def start(self, actions):
        if self.inflight:
            raise RuntimeError("step_async called again before step_wait")
        v, n = self.venv, self.n
        actions = np.asarray(actions)
        f = v._single_launch()
        if f:
            # the single-launch step reads the ego's pairs where the host wrote them: no staging copy
            if self.act is None:
                self.act = MappedBuffer(self.L, v._b._dev_index, n * 2 * 4)
                self._act_np = self.act.view().view(np.int32).reshape(n, 2)
            np.copyto(self._act_np, actions.reshape(n, 2), casting="unsafe")
            v._fast_step(f, self.act.dev, False)
        else:
            v.step_tensors(self.staged(actions))
        self._pack()
        self.inflight = True

    def finish(self):
        if not self.inflight:
            raise RuntimeError("step_wait without step_async")
        self.inflight = False
        return self._wait()

    def close(self):
        if self.inflight:               # a step nobody waited for ends first
            self._wait()
            self.inflight = False

    def _pack(self):
        self.flip ^= 1
        self.pack("oc_pack_host_tiled", self.bufs[self.flip].dev)
        self.event.record(torch.cuda.current_stream(self._words.device))

    def _wait(self):
        ev, deadline = self.event, time.monotonic() + self.timeout
        while not ev.query():
            if time.monotonic() > deadline:
                raise RuntimeError("host_io=\"mapped\": the step did not finish within %g s" % self.timeout)
        host = self.bufs[self.flip].view()
        if not self.reuse:
            return self.views(host.copy())
        # views of the two buffers are the same arrays every other step: cut them once per buffer
        cut = self._cut[self.flip]
        if cut is None:
            cut = self._cut[self.flip] = self.views(host)
        return (dict(cut[0]),) + cut[1:]


TRANSPORTS = {"copy": HostCopy, "mapped": HostMapped}      # OvercookedVecEnv(host_io=...)
