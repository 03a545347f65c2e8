#!/usr/bin/env python3
"""What the recurrent seat costs: the LSTM actor-critic step (`oc_policy_lstm_ac`, include/oc_policy.h;
`FusedRecurrentPartner`) at 4 096 and 131 072 envs, F = 29 float32 rows, C = 2.

 (a) the bare launch: 16 launches per captured graph on fixed rows, state updated in place, per launch;
 (b) GPU time per env step of a 16-step captured `ClosedLoop` whose partner is the recurrent seat with a
     fused `RolloutSink`: `RecurrentPolicyPartner` around the same `LSTMActorCritic` as torch ops against
     `FusedRecurrentPartner`.

Timing: HIP events on the launch stream around a block of graph replays, after >= 150 ms of the same
work; the median (min .. max) of 7 blocks.  Every measurement runs in a child process of its own
under a time limit, and the first one that fails ends the run.  The output kept in
profiles/recurrent_seat_rates.txt is this program's."""
import os
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, F, N_STEPS = 2, 29, 128
LIMIT = 240          # seconds per measurement
JOBS = [(what, n) for n in (4096, 131072) for what in ("launch", "loop-torch", "loop-fused")]
LABEL = {"launch": "(a) oc_policy_lstm_ac, 16 launches per replay",
         "loop-torch": "(b) ClosedLoop, 16 steps per replay, fused sink, RecurrentPolicyPartner(LSTMActorCritic as torch ops)",
         "loop-fused": "(b) ClosedLoop, 16 steps per replay, fused sink, FusedRecurrentPartner"}


def gpu_time(fn, calls, blocks=7):
    """Seconds of GPU time per call of fn: median, min, max over `blocks` event-timed blocks."""
    import torch
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


def launches(n):
    """16 launches of the kernel on fixed rows as one captured graph."""
    import torch
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic
    pol = LSTMActorCritic(3, C, seed=1).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    obs = SimpleNamespace(rows=torch.randn((F, n), generator=gen, device="cuda"),
                          timestep=torch.rand(n, generator=gen, device="cuda").double())
    act = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    seat = FusedRecurrentPartner(pol, sample=True, seed=3)
    fn = lambda: seat.act_into(obs, act[0], act[1])  # noqa: E731
    fn()
    seat.episode_start.zero_()          # the steady state: nobody starts
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(16):
            fn()
    return graph.replay


def closed_loop(n, what):
    import torch
    from gym_comm_amd.vec_env import (FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RecurrentPolicyPartner,
                                      RolloutSink)
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500, ego_config={},
                          partner_config={}, num_communication=C, communication_on=True, ego_led=False, fow_radius=2)
    sink = RolloutSink(N_STEPS, n, F, obs_dtype=torch.float32, fused=True)
    pol = LSTMActorCritic(3, C, seed=1).cuda()
    if what == "loop-torch":
        # the module masks the state itself: the seat's own mask would be five more launches per tensor
        partner = RecurrentPolicyPartner(pol, pol.initial_state(n, "cuda"), sample=True, seed=3, sink=sink, mask_state=False)
    else:
        partner = FusedRecurrentPartner(pol, sample=True, seed=3, sink=sink)
    venv = OvercookedVecEnv(arg, n, partner=partner, seed=1, obs_dtype=torch.float32)
    assert venv._b.F == F
    venv.reset_tensors()
    return venv.closed_loop(None, graph=True, steps=16).step      # the ego's rows stay as they are


def one(what, n):
    import torch
    assert torch.cuda.is_available(), "recurrent_seat_rates.py measures on a GPU"
    fn = launches(n) if what == "launch" else closed_loop(n, what)
    t = [x / 16 for x in gpu_time(fn, 200 if n <= 4096 else 40)]
    print("n=%d %s: %.2f us/%s (%.2f .. %.2f)" % (n, LABEL[what], t[0] * 1e6, "launch" if what == "launch" else "step",
                                                   t[1] * 1e6, t[2] * 1e6), flush=True)
    print("RESULT %s %d %.6e" % (what, n, t[0]), flush=True)


def main():
    got = {}
    for what, n in JOBS:
        # a fresh child per measurement, under its own time limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, str(n)], timeout=LIMIT,
                               stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired as e:       # the child has been killed and reaped
            print(e.stdout or "", end="", flush=True)
            sys.exit("measurement %s n=%d wrote no result within %d s: stopping" % (what, n, LIMIT))
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                got[(what, n)] = float(line.split()[3])
            else:
                print(line, flush=True)
        if r.returncode != 0:
            sys.exit("measurement %s n=%d ended with status %d: stopping" % (what, n, r.returncode))
        if what == "loop-fused":
            a, b = got[("loop-torch", n)], got[("loop-fused", n)]
            print("n=%d     -> the fused seat saves %.2f us/step (%.2fx)" % (n, (a - b) * 1e6, a / b), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
    else:
        main()
