#!/usr/bin/env python3
"""What a whole `train()` costs: 10 epochs over tools/ppo_update_rates.py's sink (128 x 4 096 = 524 288
samples, F = 29 float32 rows, C = 2) at minibatches of 4 096 and 16 384 --

 torch-shuffle   `PPOLearner.train(sink, 10, B)` as it was: torch.randperm and four torch ops per epoch,
                 the split on the host, one `update()` per minibatch from Python
 device-eager    `train(..., shuffle="device")`: the train sequence of include/oc_policy.h launched from
                 Python (the shuffle kernel, `oc_policy_ppo_train_step` per minibatch)
 device-graph    one `train_graph(...).replay()`: the same sequence as one captured graph

For each: wall time and GPU time of the call up to its completion (HIP events; perf_counter around a
synchronised block), and what the HOST spends inside the call before it returns -- elapsed time and
the process's CPU time -- with the synchronisation outside.  After a warm-up of the same work, the
median (min .. max) of 7 calls.  Every measurement runs in a child process of its own under a time
limit, and the first one that fails ends the run.  The output kept in profiles/ppo_train_rates.txt is
this program's."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EPOCHS, LIMIT = 10, 300
JOBS = [(what, B) for B in (4096, 16384) for what in ("torch-shuffle", "device-eager", "device-graph")]


def timed(fn, blocks=7):
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
    return med(gpu), med(wall), med(host), med(cpu)


def one(what, B):
    import torch
    import ppo_update_rates as base
    assert torch.cuda.is_available(), "ppo_train_rates.py measures on a GPU"
    sink, pol, seat, learner = base.synthetic()
    if what == "torch-shuffle":
        gen = torch.Generator(device="cuda").manual_seed(5)
        fn = lambda: learner.train(sink, n_epochs=EPOCHS, batch_size=B, generator=gen)  # noqa: E731
    elif what == "device-eager":
        fn = lambda: learner.train(sink, n_epochs=EPOCHS, batch_size=B, shuffle="device", seed=5)  # noqa: E731
    else:
        fn = learner.train_graph(sink, EPOCHS, batch_size=B, seed=5).replay
    res = timed(fn)
    st = learner.train_stats() if what != "torch-shuffle" else None
    ms = lambda r: "%.2f ms (%.2f .. %.2f)" % tuple(v * 1e3 for v in r)  # noqa: E731
    print("B=%d %s, %d epochs: wall %s, GPU %s, host in the call %s, of it CPU %s%s"
          % (B, what, EPOCHS, ms(res[1]), ms(res[0]), ms(res[2]), ms(res[3]),
             "" if st is None else "  [%d updates, %d epochs]" % (st["updates"], st["epochs"])), flush=True)
    print("RESULT %s %d %s" % (what, B, " ".join("%.6e" % r[0] for r in res)), flush=True)


def main():
    got = {}
    for what, B in JOBS:
        # a fresh child per measurement, under its own time limit; nothing more is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, str(B)], timeout=LIMIT,
                               stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired as e:       # the child has been killed and reaped
            print(e.stdout or "", end="", flush=True)
            sys.exit("measurement %s B=%d wrote no result within %d s: stopping" % (what, B, LIMIT))
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                got[(what, B)] = [float(v) for v in line.split()[3:]]
            else:
                print(line, flush=True)
        if r.returncode != 0:
            sys.exit("measurement %s B=%d ended with status %d: stopping" % (what, B, r.returncode))
        if what == "device-graph":
            t, g = got[("torch-shuffle", B)], got[("device-graph", B)]
            print("B=%d     -> train(): wall %.2f ms -> %.2f ms (%.3fx), GPU %.2f -> %.2f ms, host in the call %.2f -> %.3f ms"
                  % (B, t[1] * 1e3, g[1] * 1e3, t[1] / g[1], t[0] * 1e3, g[0] * 1e3, t[2] * 1e3, g[2] * 1e3), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
    else:
        main()
