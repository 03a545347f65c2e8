#!/usr/bin/env python3
"""What a map set costs and what it saves (BatchedOvercooked.from_maps, include/oc_hip.h: oc_mapset_*),
tomato-2 on its structure library, 16 fused steps per captured graph:

 (a) the set path's overhead: ONE map with every group on it against the single-level launch on the
     same structure library, at 4 096 and 131 072 envs, the plain step (XO = 0: four action rows) and
     the options step (XO = 1: int32 ego pairs + the in-kernel partner + episode statistics).  The
     single-level kernels of a structure library are the parent commit's, instruction for
     instruction (tools/dump_isa.py --digest), so this is also "against the parent".  At 4 096 envs
     the single-level plain step is lane-split by default (two lanes per env, oc_multi_step_lanes), a
     launch the set kernels do not have: it is shown as launched and with OC_LAUNCH=lanes=1, the
     same shape as the set's;
 (b) the reason for the feature: three maps x 4 096 envs as ONE set launch per step against three
     single-level launches per step (one batch per map) captured in the same graph.

Timing: HIP events on the launch stream around a block of graph replays, after >= 150 ms of the same
work; the median (min .. max) of 7 blocks.  The output kept in profiles/mapset_rates.txt is this program's."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gym_comm_amd import compiler
from gym_comm_amd.batched import BatchedOvercooked, pcg32_seed_states

C, STEPS, T = 2, 16, 500
MAPS = ["open-divider_tomato", "partial-divider_tomato", "full-divider_tomato"]


def gpu_time(fn, calls, blocks=7):
    """Seconds of GPU time per call of fn: median, min, max over `blocks` event-timed blocks."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(blocks):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e-3 / calls)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def show(what, t):
    t = tuple(x / STEPS for x in t)
    print("%s: %.3f us/step (%.3f .. %.3f)" % (what, t[0] * 1e6, t[1] * 1e6, t[2] * 1e6), flush=True)
    return t[0]


class Stepper:
    """One batch and the tensors its step reads: step() enqueues one fused step."""

    def __init__(self, make, n, xo, seed):
        self.env = make(n, bool(xo))
        g = torch.Generator().manual_seed(seed)
        acts = torch.stack([torch.randint(0, 4, (n,), generator=g), torch.randint(0, C, (n,), generator=g)] * 2)
        self.acts = acts.to(torch.int32).cuda()
        self.pairs = self.acts[0:2].T.contiguous()
        self.rng = pcg32_seed_states(seed, (n,), "cuda")
        self.played = torch.zeros((2, n), dtype=torch.int32, device="cuda")
        self.xo = xo

    def step(self):
        if self.xo:
            self.env.multi_step(None, ego_pairs=self.pairs, alt_rng=self.rng, alt_played=self.played)
        else:
            self.env.multi_step(self.acts)


def capture(steppers, launch=None):
    """STEPS steps of every stepper, in turn, as one graph.  `launch`: OC_LAUNCH while capturing (the
    library reads it at every call; a captured launch keeps the kernel it was captured with)."""
    old = os.environ.pop("OC_LAUNCH", None)
    if launch:
        os.environ["OC_LAUNCH"] = launch
    try:
        for s in steppers:
            s.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(STEPS):
                for s in steppers:
                    s.step()
    finally:
        os.environ.pop("OC_LAUNCH", None)
        if old is not None:
            os.environ["OC_LAUNCH"] = old
    return graph


def single(level):
    lv = compiler.compile_level(level, 2, T)
    return lambda n, stats: BatchedOvercooked(lv, num_envs=n, num_communication=C, specialize_level="structure",
                                              episode_stats=stats)


def as_set(levels, **kw):
    lvs = [compiler.compile_level(m, 2, T) for m in levels]
    return lambda n, stats: BatchedOvercooked.from_maps(lvs, num_envs=n, num_communication=C, episode_stats=stats, **kw)


def main():
    assert torch.cuda.is_available(), "mapset_rates.py measures on a GPU"
    print("(a) one map, every group on it, against the single-level launch (structure library)")
    for n in (4096, 131072):
        calls = 100 if n <= 4096 else 20
        for xo in (0, 1):
            one = Stepper(single(MAPS[0]), n, xo, 1)
            many = Stepper(as_set(MAPS[:1]), n, xo, 1)
            tag = "n=%d XO=%d" % (n, xo)
            waves, lanes = one.env.launch_waves(general=bool(xo)), one.env.launch_lanes(general=bool(xo))
            base = show("%s single level (%d waves per 64 envs, %d lane%s per env)"
                        % (tag, waves, lanes, "" if lanes == 1 else "s"), gpu_time(capture([one]).replay, calls))
            if lanes != 1:
                base = show("%s single level, OC_LAUNCH=lanes=1" % tag, gpu_time(capture([one], "lanes=1").replay, calls))
            t = show("%s map set        (%d waves per 64 envs)" % (tag, many.env.launch_waves(general=bool(xo))),
                     gpu_time(capture([many]).replay, calls))
            print("%s     -> set / single level of the same launch shape = %.3f" % (tag, t / base), flush=True)
    print("(b) three maps x 4 096 envs: one set launch per step against three single-level launches per step")
    for xo in (0, 1):
        three = [Stepper(single(m), 4096, xo, 2 + k) for k, m in enumerate(MAPS)]
        many = Stepper(as_set(MAPS, envs_per_map=[4096] * 3), 3 * 4096, xo, 2)
        tag = "3 x 4096 XO=%d" % xo
        a = show("%s three launches (as launched: %d lanes per env)" % (tag, three[0].env.launch_lanes(general=bool(xo))),
                 gpu_time(capture(three).replay, 100))
        b = show("%s three launches, OC_LAUNCH=lanes=1" % tag, gpu_time(capture(three, "lanes=1").replay, 100))
        c = show("%s one set launch (%d waves per 64 envs)" % (tag, many.env.launch_waves(general=bool(xo))),
                 gpu_time(capture([many]).replay, 100))
        print("%s     -> one launch / three launches = %.3f (as launched), %.3f (lanes=1)" % (tag, c / a, c / b), flush=True)


if __name__ == "__main__":
    main()
