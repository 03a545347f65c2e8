#!/usr/bin/env python3
"""What a whole `RecurrentPPOLearner.train()` costs: 10 epochs over tools/recurrent_ppo_rates.py's sink (T = 128
steps x n = 4 096 envs, F = 29 float32 rows, C = 2) at minibatches of 1 024 and 4 096 whole sequences --

 torch-shuffle   `train(sink, 10, E)` as it was: torch.randperm and four torch ops per epoch, the split on the
                 host, one `update()` per minibatch from Python
 device-eager    `train(..., shuffle="device")`: the train sequence of include/oc_policy.h launched from Python
                 (the shuffle kernel, `oc_policy_recurrent_train_step` per minibatch)
 device-graph    one `train_graph(...).replay()`: the same sequence as one captured graph

For each: wall time and GPU time of the call up to its completion (HIP events; perf_counter around a
synchronised block), the GPU time per minibatch update (the call's GPU time over its updates), and what the HOST
spends inside the call before it returns -- elapsed time and the process's CPU time -- with the synchronisation
outside.  After a warm-up of the same work, the median (min .. max) of 5 calls.  Every measurement runs in a
child process of its own under a time limit, and the first one that fails ends the run.

The run-to-run spread the device variants' GPU time per update is held against: a run is a child process (its
own allocations and addresses, the clocks wherever the run before left them), and the three variants cannot
share one.  So torch-shuffle is measured in TWO processes per size, before and after the other two, and its
spread is max - min of the GPU time per update over the 10 calls of both; the figure the others are compared
with is the median of those 10.  (The 5 calls of ONE process agree far more closely than two processes do, and
say nothing about a difference between processes.)
The output kept in profiles/recurrent_ppo_train_rates.txt is this program's."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EPOCHS, LIMIT, BLOCKS = 10, 300, 5
JOBS = [(what, E) for E in (1024, 4096) for what in ("torch-shuffle", "device-eager", "device-graph", "torch-shuffle")]


def timed(fn, blocks=BLOCKS):
    """Medians with (min, max) over `blocks` calls of fn: GPU seconds, wall seconds to completion, host
    seconds until fn returns, host CPU seconds until fn returns."""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gpu, wall, host, cpu = [], [], [], []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0, c0 = time.perf_counter(), time.process_time()
        e0.record()
        fn()
        t1, c1 = time.perf_counter(), time.process_time()
        e1.record()
        e1.synchronize()
        wall.append(time.perf_counter() - t0)
        gpu.append(e0.elapsed_time(e1) * 1e-3)
        host.append(t1 - t0)
        cpu.append(c1 - c0)
    med = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))  # noqa: E731
    return med(gpu), med(wall), med(host), med(cpu), gpu


def one(what, E):
    import torch
    import recurrent_ppo_rates as base
    assert torch.cuda.is_available(), "recurrent_ppo_train_rates.py measures on a GPU"
    sink, pol, seat, learner = base.synthetic()
    updates = EPOCHS * len(learner.minibatches(sink, E))
    if what == "torch-shuffle":
        gen = torch.Generator(device="cuda").manual_seed(5)
        fn = lambda: learner.train(sink, n_epochs=EPOCHS, envs_per_batch=E, generator=gen)  # noqa: E731
    elif what == "device-eager":
        fn = lambda: learner.train(sink, n_epochs=EPOCHS, envs_per_batch=E, shuffle="device", seed=5)  # noqa: E731
    else:
        fn = learner.train_graph(sink, EPOCHS, envs_per_batch=E, seed=5).replay
    res = timed(fn)
    if what != "torch-shuffle":
        st = learner.train_stats()
        assert st["updates"] == updates and st["epochs"] == EPOCHS and not st["stopped"], st
    assert int(learner.step.item()) == updates * (BLOCKS + 1)
    ms = lambda r: "%.2f ms (%.2f .. %.2f)" % tuple(v * 1e3 for v in r)  # noqa: E731
    per = tuple(v / updates for v in res[0])
    print("E=%d %s, %d epochs, %d updates: wall %s, GPU %s = %.1f us/update (%.1f .. %.1f), host in the call %s, of it CPU %s"
          % (E, what, EPOCHS, updates, ms(res[1]), ms(res[0]), per[0] * 1e6, per[1] * 1e6, per[2] * 1e6, ms(res[2]),
             ms(res[3])), flush=True)
    print("RESULT %s %d %s %.6e" % (what, E, " ".join("%.6e" % r[0] for r in res[:4]), per[0]), flush=True)
    print("CALLS %s" % " ".join("%.6e" % (v / updates) for v in res[4]), flush=True)


def main():
    got, calls = {}, {}
    for what, E in JOBS:
        # a fresh child per measurement, under its own time limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, str(E)], timeout=LIMIT,
                               stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired as e:       # the child has been killed and reaped
            print(e.stdout or "", end="", flush=True)
            sys.exit("measurement %s E=%d wrote no result within %d s: stopping" % (what, E, LIMIT))
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                got.setdefault((what, E), [float(v) for v in line.split()[3:]])      # (torch-shuffle: its first run's)
            elif line.startswith("CALLS "):
                calls.setdefault((what, E), []).extend(float(v) for v in line.split()[1:])
            else:
                print(line, flush=True)
        if r.returncode != 0:
            sys.exit("measurement %s E=%d ended with status %d: stopping" % (what, E, r.returncode))
        if what == "torch-shuffle" and len(calls[(what, E)]) > BLOCKS:          # its second run: the size is complete
            t, d, g = got[("torch-shuffle", E)], got[("device-eager", E)], got[("device-graph", E)]
            print("E=%d     -> train(): wall %.2f ms -> %.2f ms (%.3fx), host in the call %.2f -> %.3f ms" %
                  (E, t[1] * 1e3, g[1] * 1e3, t[1] / g[1], t[2] * 1e3, g[2] * 1e3), flush=True)
            both = sorted(calls[(what, E)])
            base, spread = both[len(both) // 2], both[-1] - both[0]
            print("E=%d     -> GPU per update: torch-shuffle %.1f us over its two runs (spread %.1f us: %.1f .. %.1f), "
                  "device-eager %+.1f us, device-graph %+.1f us against it: %s"
                  % (E, base * 1e6, spread * 1e6, both[0] * 1e6, both[-1] * 1e6, (d[4] - base) * 1e6, (g[4] - base) * 1e6,
                     "within the spread" if max(d[4], g[4]) - base <= spread else "ABOVE the spread"), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
    else:
        main()
