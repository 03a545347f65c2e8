#!/usr/bin/env python3
"""What windows cost and give: the state snapshot in the closed loop (`oc_policy_window_snapshot`) and the recurrent
update over WINDOWS of a rollout (`oc_policy_window_gather` in front of the unchanged `oc_policy_rppo_update`,
include/oc_policy.h) against the same work over whole sequences, F = 29 float32 rows, C = 2.

 (a) loop     GPU time per env step of a 16-step captured `ClosedLoop` whose partner is `FusedRecurrentPartner` with a
              fused `RolloutSink` of 128 steps, at 4 096 and 131 072 envs: without windows, and recording the state
              every 16 steps (`state_window=16`)
 (b) update   T = 128, n = 4 096, ONE captured update of 131 072 samples: 1 024 whole sequences (`update`), 8 192 windows
              of 16 and 4 096 windows of 32 (`update_windows`); and the same update under torch's profiler: GPU time of
              the forward, the backward and the gather (the mean of 5 eager updates)
 (c) train    the same three ways, one replay of a captured 10-epoch train sequence (`train_graph`, 4 minibatches per epoch)

`--parent DIR`: a built checkout of the commit before windows existed; the runs without windows are then made on
THAT tree (its package, its libraries), in the same session, alternating with this tree's.  Without it they are
made on this tree with `state_window=None` and labelled so.

Timing: HIP events around graph replays after a warm-up of the same work; the median (min .. max) of the blocks.
Every figure is taken in TWO processes: the spread printed is the difference of their medians.  Every measurement
runs in a child process of its own under a time limit, and the first one that fails ends the run.  The output kept
in profiles/recurrent_window_rates.txt is this program's."""
import argparse
import os
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, F, T, N = 2, 29, 128, 4096
SAMPLES = 131072
EPOCHS = 10
LIMIT = 300
HP = dict(lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)


def gpu_time(fn, calls, blocks=7, warm=0.15):
    """Seconds of GPU time per call of fn: median, min, max over `blocks` event-timed blocks."""
    import torch
    t0 = time.perf_counter()
    fn()
    while time.perf_counter() - t0 < warm:
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


def loop(n, W):
    import torch
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RolloutSink
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500, ego_config={},
                          partner_config={}, num_communication=C, communication_on=True, ego_led=False, fow_radius=2)
    kw = {} if W is None else {"state_window": W}
    sink = RolloutSink(T, n, F, obs_dtype=torch.float32, fused=True, **kw)
    pol = LSTMActorCritic(3, C, seed=1).cuda()
    partner = FusedRecurrentPartner(pol, sample=True, seed=3, sink=sink)
    venv = OvercookedVecEnv(arg, n, partner=partner, seed=1, obs_dtype=torch.float32)
    assert venv._b.F == F
    venv.reset_tensors()
    step = venv.closed_loop(None, graph=True, steps=16).step
    t = [x / 16 for x in gpu_time(step, 200 if n <= 4096 else 40)]
    print("RESULT loop %.6e %.6e %.6e" % tuple(t), flush=True)


def synthetic(W):
    """A full fused sink of random rows recorded by the seat's own kernels, the seat and a learner."""
    import torch
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic, RecurrentPPOLearner, RolloutSink
    gen = torch.Generator(device="cuda").manual_seed(1)
    kw = {} if W is None else {"state_window": W}
    sink = RolloutSink(T, N, F, obs_dtype=torch.float32, fused=True, **kw)
    pol = LSTMActorCritic(3, C, seed=1).cuda()
    seat = FusedRecurrentPartner(pol, sample=True, seed=3, sink=sink)
    seat.begin_rollout(N)
    mv, cm = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    for s in range(T):
        obs = SimpleNamespace(rows=torch.randint(-2, 3, (F, N), generator=gen, device="cuda").float(),
                              timestep=torch.rand(N, generator=gen, device="cuda").double())
        seat.act_into(obs, mv, cm)
        done = (torch.rand(N, generator=gen, device="cuda") < 0.01).int()
        seat.update(torch.randn(N, generator=gen, device="cuda").double(), done)
    seat.finish_rollout()
    assert sink.steps() == T and int(sink.pos.item()) == 0
    return sink, seat, RecurrentPPOLearner(seat, **HP)


def minibatch(learner, sink, W):
    """(the update of one minibatch of SAMPLES samples as a callable, sequences per minibatch)."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(5)
    if W is None:
        E = SAMPLES // T
        envs = learner.minibatches(sink, E, generator=gen)[0]
        return (lambda: learner.update(sink, envs)), E
    E = SAMPLES // W
    seqs = learner.minibatches_windows(sink, E, generator=gen)[0]
    return (lambda: learner.update_windows(sink, seqs)), E


def update(W, profiled):
    import torch
    sink, seat, learner = synthetic(W)
    fn, E = minibatch(learner, sink, W)
    fn()
    torch.cuda.synchronize()
    if profiled:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        total = {}
        for ev in prof.key_averages():
            for part in ("k_rppo_forward", "k_rppo_backward", "k_rppo_wgrad", "k_rppo_adv", "k_rppo_reduce", "k_rppo_finish",
                         "k_window_gather"):
                if part in ev.key:
                    us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    total[part] = total.get(part, 0.0) + us
        for part, us in total.items():
            print("RESULT kernel %s %.6e" % (part, us / 5.0 * 1e-6), flush=True)
        return
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    print("RESULT update %.6e %.6e %.6e" % gpu_time(graph.replay, 10), flush=True)
    plan = learner.plan(E, T if W is None else W)
    print("RESULT plan %d %d %.1f" % (plan[0], plan[1], plan[4] * 4 / 1e6), flush=True)
    if W is None:
        tg = learner.train_graph(sink, EPOCHS, envs_per_batch=E)
    else:
        tg = learner.train_graph_windows(sink, EPOCHS, sequences_per_batch=E)
    print("RESULT train %.6e %.6e %.6e" % gpu_time(tg.replay, 1, blocks=3, warm=0.0), flush=True)
    st = learner.train_stats()
    assert st["updates"] == EPOCHS * (T * N // SAMPLES) and not st["stopped"], st


def child(argv):
    import torch
    assert torch.cuda.is_available(), "recurrent_window_rates.py measures on a GPU"
    what, W = argv[0], None if argv[1] == "none" else int(argv[1])
    if what == "loop":
        loop(int(argv[2]), W)
    else:
        update(W, what == "kernels")


def run(root, *args):
    """One measurement in a fresh child on the package under `root`; {name: [floats]} of its RESULT lines."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root] + [str(a) for a in args],
                           timeout=LIMIT, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:           # the child has been killed and reaped
        print(e.stdout or "", end="", flush=True)
        sys.exit("measurement %s wrote no result within %d s: stopping" % (args, LIMIT))
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            w = line.split()
            key = w[1] if w[1] != "kernel" else w[2]
            out[key] = [float(x) for x in (w[2:] if w[1] != "kernel" else w[3:])]
        else:
            print(line, flush=True)
    if r.returncode != 0:
        sys.exit("measurement %s ended with status %d: stopping" % (args, r.returncode))
    return out


def twice(jobs):
    """Every job of `jobs` ({label: (root, args)}) in two processes, the jobs alternating; {label: [out, out]}."""
    got = {k: [] for k in jobs}
    for _ in range(2):
        for k, (root, args) in jobs.items():
            got[k].append(run(root, *args))
    return got


def fmt(pair, key, unit=1e6):
    a, b = pair[0][key], pair[1][key]
    return "%.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f); spread %.2f" % (
        a[0] * unit, a[1] * unit, a[2] * unit, b[0] * unit, b[1] * unit, b[2] * unit, abs(a[0] - b[0]) * unit)


def mean(pair, key):
    return 0.5 * (pair[0][key][0] + pair[1][key][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the commit before windows existed")
    a = ap.parse_args()
    base = os.path.abspath(a.parent) if a.parent else ROOT
    whose = "the parent commit's tree" if a.parent else "THIS tree with state_window=None (no parent tree given)"
    print("runs without windows: %s.  Each figure: process 1 | process 2, median (min .. max); spread = |difference of "
          "the medians|" % whose, flush=True)
    print("(a) 16-step captured closed loop, FusedRecurrentPartner + fused sink of %d steps, us per env step" % T, flush=True)
    for n in (4096, 131072):
        got = twice({"without": (base, ("loop", "none", n)), "window16": (ROOT, ("loop", 16, n))})
        print("n=%-6d without windows        %s" % (n, fmt(got["without"], "loop")), flush=True)
        print("n=%-6d state_window=16        %s" % (n, fmt(got["window16"], "loop")), flush=True)
        d = (mean(got["window16"], "loop") - mean(got["without"], "loop")) * 1e6
        sp = abs(got["without"][0]["loop"][0] - got["without"][1]["loop"][0]) * 1e6
        print("n=%-6d     -> the snapshot costs %+.2f us per step (the means of the two processes); the spread of the "
              "loop without it is %.2f us: %s" % (n, d, sp, "within it" if abs(d) <= sp else "ABOVE it" if d > 0 else "below it"),
              flush=True)
    print("(b), (c) T = %d, n = %d, minibatches of %d samples; (b) us per captured update, (c) ms per replay of a captured "
          "%d-epoch train (%d updates)" % (T, N, SAMPLES, EPOCHS, EPOCHS * T * N // SAMPLES), flush=True)
    jobs = {"whole": (base, ("update", "none")), "w16": (ROOT, ("update", 16)), "w32": (ROOT, ("update", 32))}
    label = {"whole": "%d whole sequences  " % (SAMPLES // T), "w16": "%d windows of 16   " % (SAMPLES // 16),
             "w32": "%d windows of 32   " % (SAMPLES // 32)}
    got = twice(jobs)
    for k in jobs:
        p = got[k][0]["plan"]
        print("(b) %s %s; forward / backward workgroups %d, scratch %.1f MB" % (label[k], fmt(got[k], "update"), p[0], p[2]),
              flush=True)
    for k in jobs:
        print("(c) %s %s" % (label[k], fmt(got[k], "train", 1e3)), flush=True)
    for k in ("w16", "w32"):
        print("    -> %s against whole sequences: update %.2fx, train %.2fx (ratios of the means; above 1 = windows faster)"
              % (label[k].strip(), mean(got["whole"], "update") / mean(got[k], "update"),
                 mean(got["whole"], "train") / mean(got[k], "train")), flush=True)
    print("(b) per kernel, us per update, under torch's profiler (one process each)", flush=True)
    for k, (root, args) in jobs.items():
        ker = run(root, "kernels", args[1])
        print("    %s %s" % (label[k], "  ".join("%s %.1f" % (name.replace("k_rppo_", "").replace("k_window_", ""), v[0] * 1e6)
                                                   for name, v in sorted(ker.items(), key=lambda kv: -kv[1][0]))), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        sys.path.insert(0, sys.argv[2])
        child(sys.argv[3:])
    else:
        main()
