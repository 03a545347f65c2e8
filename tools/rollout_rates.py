#!/usr/bin/env python3
"""What the rollout buffer costs beside the step: `RolloutSink` as torch ops (`fused=False`) against
`liboc_rollout.so` (`fused=True`, include/oc_rollout.h), at 4 096 and 131 072 envs, F = 29 float32 rows.

 (a) GPU time per env step of a 16-step captured `ClosedLoop` with a `RecurrentPolicyPartner` whose
     policy is one linear layer: without a sink, with the torch sink, with the fused sink;
 (a') the recording alone: 16 `add` + `add_reward` pairs as one captured graph, per pair;
 (b) `compute_returns_and_advantage` at n_steps = 128: the torch loop against the kernel.

Timing: HIP events on the launch stream around a block of calls, after >= 150 ms of the same work;
the median (min .. max) of 7 blocks.  The output kept in profiles/rollout_rates.txt is this program's."""
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gym_comm_amd.vec_env import OvercookedVecEnv, RecurrentPolicyPartner, RolloutSink

C, N_STEPS = 2, 128


class LinearPolicy(torch.nn.Module):
    """One GEMM on the [F][n] rows as they lie: 4 move logits, C comm logits and a value."""
    feature_major = True

    def __init__(self, F):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.w = torch.nn.Parameter((torch.rand((4 + C + 1, F), generator=g) - 0.5) * 0.1)

    def forward(self, obs, state, episode_start):
        out = self.w @ obs.rows
        return out[:4], out[4:4 + C], state, out[4 + C]


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


def show(n, what, t, unit="step"):
    print("n=%d %s: %.2f us/%s (%.2f .. %.2f)" % (n, what, t[0] * 1e6, unit, t[1] * 1e6, t[2] * 1e6), flush=True)
    return t[0]


def closed_loop(n, sink_kind):
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500, ego_config={},
                          partner_config={}, num_communication=C, communication_on=True, ego_led=False,
                          fow_radius=2)
    F = 22 + 3 + 2 * C
    sink = None if sink_kind is None else RolloutSink(N_STEPS, n, F, obs_dtype=torch.float32,
                                                      fused=sink_kind == "fused")
    partner = RecurrentPolicyPartner(LinearPolicy(F).cuda(), torch.zeros(n, 1, device="cuda"), sample=True, seed=3,
                                     sink=sink, mask_state=False)
    venv = OvercookedVecEnv(arg, n, partner=partner, seed=1, obs_dtype=torch.float32)
    assert venv._b.F == F
    venv.reset_tensors()
    loop = venv.closed_loop(None, graph=True, steps=16)      # the ego's rows stay as they are
    return loop


def recording_alone(n, fused):
    F = 29
    sink = RolloutSink(N_STEPS, n, F, obs_dtype=torch.float32, fused=fused)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.randn((F, n), generator=gen, device="cuda")
    ts = torch.zeros(n, dtype=torch.float64, device="cuda")
    act = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    f32 = torch.randn((3, n), generator=gen, device="cuda")
    rew = torch.zeros(n, dtype=torch.float64, device="cuda")
    done = torch.zeros(n, dtype=torch.int32, device="cuda")

    def pair():
        sink.add(rows, ts, act[0], act[1], f32[0], f32[1], f32[2])
        sink.add_reward(rew, done)
    pair()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(16):
            pair()
    return graph


def gae(n, fused):
    sink = RolloutSink(N_STEPS, n, 1, obs_dtype=torch.float32, fused=fused)
    gen = torch.Generator(device="cuda").manual_seed(2)
    sink.rewards.copy_(torch.randn((N_STEPS, n), generator=gen, device="cuda", dtype=torch.float64))
    sink.values.copy_(torch.randn((N_STEPS, n), generator=gen, device="cuda"))
    sink.episode_starts.copy_((torch.rand((N_STEPS, n), generator=gen, device="cuda") < 0.02).float())
    sink.count.fill_(N_STEPS)
    lv = torch.randn(n, generator=gen, device="cuda")
    ld = torch.zeros(n, device="cuda")
    return sink, (lambda: sink.compute_returns_and_advantage(lv, ld))


def main():
    assert torch.cuda.is_available(), "rollout_rates.py measures on a GPU"
    for n in (4096, 131072):
        calls = 200 if n <= 4096 else 40
        base = None
        for kind in (None, "torch", "fused"):
            loop = closed_loop(n, kind)
            t = gpu_time(loop.step, calls)
            t = show(n, "(a) ClosedLoop, 16 steps per replay, linear RecurrentPolicyPartner, %s"
                     % {None: "no sink", "torch": "torch sink", "fused": "fused sink"}[kind],
                     tuple(x / 16 for x in t))
            if kind is None:
                base = t
            else:
                print("n=%d     -> recording adds %.2f us/step" % (n, (t - base) * 1e6), flush=True)
        for fused in (False, True):
            graph = recording_alone(n, fused)
            show(n, "(a') add + add_reward alone, 16 pairs per replay, %s" % ("fused" if fused else "torch"),
                 tuple(x / 16 for x in gpu_time(graph.replay, calls)), "pair")
        res = {}
        for fused in (False, True):
            sink, fn = gae(n, fused)
            res[fused] = (sink, show(n, "(b) compute_returns_and_advantage, n_steps=%d, %s"
                                     % (N_STEPS, "kernel" if fused else "torch loop"),
                                     gpu_time(fn, 50 if fused else 3, blocks=5), "call"))
        same = all(torch.equal(getattr(res[True][0], f).view(torch.int32), getattr(res[False][0], f).view(torch.int32))
                   for f in ("advantages", "returns"))
        print("n=%d     -> torch loop / kernel = %.0fx, outputs bit-identical: %s"
              % (n, res[False][1] / res[True][1], same), flush=True)


if __name__ == "__main__":
    main()
