#!/usr/bin/env python3
"""What the recurrent learner's update costs: `RecurrentPPOLearner.update` (six launches: `oc_policy_rppo_update`,
include/oc_policy.h) against the same minibatch as torch ops, on a 128 x 4 096 sink, F = 29 float32 rows,
C = 2, at minibatches of E = 1 024 and E = 4 096 whole sequences (131 072 and 524 288 samples).

 fused-graph   one `update` captured into a graph: GPU time per replay
 fused-kernels the same update under torch's profiler: GPU time per kernel (the mean of 5 eager updates)
 torch         `LSTMActorCritic` unrolled over the 128 steps as torch ops, the loss of include/oc_policy.h,
               autograd, `clip_grad_norm_`, `torch.optim.Adam.step`, `seat.refresh()`: GPU and wall time

Timing: after a warm-up of the same work, HIP events (GPU time) and perf_counter around a synchronised block
(wall time); the median (min .. max) of 7 blocks (3 for torch).  Every measurement runs in a child process of
its own under a time limit, and the first one that fails ends the run.  The output kept in
profiles/recurrent_ppo_rates.txt is this program's."""
import os
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, F, T, N = 2, 29, 128, 4096
LIMIT = 300
JOBS = [(what, E) for E in (1024, 4096) for what in ("fused-graph", "fused-kernels", "torch")]
HP = dict(lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)


def timed(fn, blocks=7):
    """(GPU seconds, wall seconds) of one call of fn: medians, with (min, max), over `blocks` calls."""
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    gpu, wall = [], []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append(time.perf_counter() - t0)
        gpu.append(e0.elapsed_time(e1) * 1e-3)
    med = lambda v: (sorted(v)[len(v) // 2], min(v), max(v))  # noqa: E731
    return med(gpu), med(wall)


def synthetic():
    """A full fused sink of random rows recorded by the seat's own kernel, the seat and a learner."""
    import torch
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic, RecurrentPPOLearner, RolloutSink
    gen = torch.Generator(device="cuda").manual_seed(1)
    sink = RolloutSink(T, N, F, obs_dtype=torch.float32, fused=True)
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
    return sink, pol, seat, RecurrentPPOLearner(seat, **HP)


class TorchUpdate:
    """The update as torch ops on the module, the seat refreshed after every minibatch."""

    def __init__(self, pol, seat):
        import torch
        self.pol, self.seat = pol, seat
        self.opt = torch.optim.Adam(pol.parameters(), lr=HP["lr"], eps=1e-5)

    def __call__(self, sink, envs):
        import torch
        i = envs.long()
        h, c = self.seat.h0[:, i].T, self.seat.c0[:, i].T
        lps, vals, ents = [], [], []
        for t in range(sink.obs.shape[0]):
            obs = SimpleNamespace(rows=sink.obs[t][:, i], timestep=sink.timestep[t][i])
            mv, cm, (h, c), value = self.pol(obs, (h, c), sink.episode_starts[t][i])
            a = sink.actions[t][:, i].long()
            lp, H = 0.0, 0.0
            for logits, col in ((mv, 0), (cm, 1)):
                ls = torch.log_softmax(logits, dim=0)
                lp = lp + ls.gather(0, a[col].reshape(1, -1)).reshape(-1)
                H = H - (ls.exp() * ls).sum(dim=0)
            lps.append(lp), vals.append(value), ents.append(H)
        lp, value, H = torch.stack(lps), torch.stack(vals), torch.stack(ents)
        adv = sink.advantages[:, i]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(lp - sink.log_probs[:, i])
        c_ = HP["clip_range"]
        pol_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c_, 1 + c_)).mean()
        val_loss = ((sink.returns[:, i] - value) ** 2).mean()
        loss = pol_loss + HP["ent_coef"] * (-H.mean()) + HP["vf_coef"] * val_loss
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.pol.parameters(), HP["max_grad_norm"])
        self.opt.step()
        self.seat.refresh()


def one(what, E):
    import torch
    assert torch.cuda.is_available(), "recurrent_ppo_rates.py measures on a GPU"
    sink, pol, seat, learner = synthetic()
    envs = learner.minibatches(sink, E, generator=torch.Generator(device="cuda").manual_seed(5))[0]
    plan = learner.plan(E, T)
    if what == "fused-graph":
        learner.update(sink, envs)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            learner.update(sink, envs)
        (g, glo, ghi), (w, _, _) = timed(graph.replay)
        print("E=%d (%d samples) fused, captured: GPU %.1f us/update (%.1f .. %.1f); scratch %.1f MB (%d floats per sample); "
              "workgroups: forward / backward %d, weight gradient %d"
              % (E, E * T, g * 1e6, glo * 1e6, ghi * 1e6, plan[4] * 4 / 1e6, plan[7], plan[0], plan[1]), flush=True)
    elif what == "fused-kernels":
        from torch.profiler import ProfilerActivity, profile
        learner.update(sink, envs)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                learner.update(sink, envs)
            torch.cuda.synchronize()
        rows = [(ev.key, getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0), ev.count)
                for ev in prof.key_averages() if "k_rppo_" in ev.key]
        total = sum(us for _, us, _ in rows) / 5.0
        for key, us, count in sorted(rows, key=lambda r: -r[1]):
            name = key[key.index("k_rppo_"):].split("(")[0].split("E")[0]
            print("E=%d   %-18s %9.1f us/update (%4.1f %%), %d launch(es) per update"
                  % (E, name, us / 5.0, 100.0 * us / 5.0 / max(total, 1e-9), count // 5), flush=True)
        g, w = total * 1e-6, 0.0
    else:
        step = TorchUpdate(pol, seat)
        (g, glo, ghi), (w, wlo, whi) = timed(lambda: step(sink, envs), blocks=3)
        print("E=%d torch ops + autograd + Adam: GPU %.1f us/update (%.1f .. %.1f), wall %.1f us/update (%.1f .. %.1f)"
              % (E, g * 1e6, glo * 1e6, ghi * 1e6, w * 1e6, wlo * 1e6, whi * 1e6), flush=True)
    print("RESULT %s %d %.6e %.6e" % (what, E, g, w), flush=True)


def main():
    got = {}
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
                got[(what, E)] = (float(line.split()[3]), float(line.split()[4]))
            else:
                print(line, flush=True)
        if r.returncode != 0:
            sys.exit("measurement %s E=%d ended with status %d: stopping" % (what, E, r.returncode))
        if what == "torch":
            t, g = got[("torch", E)], got[("fused-graph", E)]
            print("E=%d     -> GPU: torch %.1f us, fused captured %.1f us (%.1fx)" % (E, t[0] * 1e6, g[0] * 1e6, t[0] / g[0]),
                  flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
    else:
        main()
