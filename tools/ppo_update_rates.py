#!/usr/bin/env python3
"""What the learner's update costs: `PPOLearner.update` (three launches: `oc_policy_ppo_update`,
include/oc_policy.h) against the same update as torch ops, on a 128 x 4 096 sink (524 288 samples),
F = 29 float32 rows, C = 2, at minibatches of 4 096 and 16 384.

 fused-eager   `update()` per minibatch from Python: wall time and GPU time per update
 fused-graph   one epoch of updates captured into one graph: GPU time per update
 torch         what the module offers without the learner: gather -> `forward_ac` -> the loss of
               include/oc_policy.h -> `backward` -> `clip_grad_norm_` -> `torch.optim.Adam.step` ->
               `seat.refresh()` (a device synchronisation): wall time and GPU time per update
 round-*       a whole collect-and-train round at 4 096 envs: 128 steps of a 16-step captured
               `ClosedLoop`, `finish_rollout`, 10 epochs at 16 384 (320 updates): wall time

Timing: after a warm-up of the same work, HIP events (GPU time) and perf_counter around a
synchronised block (wall time); the median (min .. max) of 7 blocks.  Every measurement runs in a
child process of its own under a time limit, and the first one that fails ends the run.  The output
kept in profiles/ppo_update_rates.txt is this program's."""
import os
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, F, T, N = 2, 29, 128, 4096
LIMIT = 300
JOBS = [(what, B) for B in (4096, 16384) for what in ("fused-eager", "fused-graph", "torch")] + \
       [("round-fused", 16384), ("round-torch", 16384)]
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
    """A full fused sink of random rows scored by a slightly different module, a seat and a learner."""
    import torch
    from gym_comm_amd.vec_env import FusedActorCriticPartner, MLPActorCritic, PPOLearner, RolloutSink
    gen = torch.Generator(device="cuda").manual_seed(1)
    sink = RolloutSink(T, N, F, obs_dtype=torch.float32, fused=True)
    sink.obs.copy_(torch.randint(-2, 3, (T, F, N), generator=gen, device="cuda").float())
    sink.timestep.copy_(torch.rand((T, N), generator=gen, device="cuda").double())
    sink.actions[:, 0].copy_(torch.randint(0, 4, (T, N), generator=gen, device="cuda"))
    sink.actions[:, 1].copy_(torch.randint(0, C, (T, N), generator=gen, device="cuda"))
    sink.advantages.copy_(torch.randn((T, N), generator=gen, device="cuda"))
    sink.returns.copy_(torch.randn((T, N), generator=gen, device="cuda"))
    old = FusedActorCriticPartner(MLPActorCritic(3, C, seed=2).cuda(), sample=False)
    for s in range(T):
        lp, v = old.score(SimpleNamespace(rows=sink.obs[s], timestep=sink.timestep[s]), sink.actions[s].T.contiguous())
        sink.log_probs[s].copy_(lp)
        sink.values[s].copy_(v)
    sink.count.fill_(T)
    sink.returns_ready = True
    pol = MLPActorCritic(3, C, seed=1).cuda()
    seat = FusedActorCriticPartner(pol, sample=True, seed=3)
    return sink, pol, seat, PPOLearner(seat, **HP)


class TorchUpdate:
    """The update as torch ops on the module, the seat refreshed after every minibatch."""

    def __init__(self, pol, seat):
        import torch
        self.pol, self.seat = pol, seat
        self.opt = torch.optim.Adam(pol.parameters(), lr=HP["lr"], eps=1e-5)

    def __call__(self, sink, idx):
        import torch
        n = sink.obs.shape[2]
        i = idx.long()
        slot, env = i // n, i % n
        obs = SimpleNamespace(rows=sink.obs[slot, :, env].T, timestep=sink.timestep.reshape(-1)[i])
        mv, cm, value = self.pol.forward_ac(obs)
        a = sink.actions[slot, :, env].long()
        lp, H = 0.0, 0.0
        for logits, col in ((mv, 0), (cm, 1)):
            ls = torch.log_softmax(logits, dim=0)
            lp = lp + ls.gather(0, a[:, col].reshape(1, -1)).reshape(-1)
            H = H - (ls.exp() * ls).sum(dim=0)
        adv = sink.advantages.reshape(-1)[i]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(lp - sink.log_probs.reshape(-1)[i])
        c = HP["clip_range"]
        pol_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        val_loss = ((sink.returns.reshape(-1)[i] - value) ** 2).mean()
        loss = pol_loss + HP["ent_coef"] * (-H.mean()) + HP["vf_coef"] * val_loss
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.pol.parameters(), HP["max_grad_norm"])
        self.opt.step()
        self.seat.refresh()


def updates(what, B):
    import torch
    sink, pol, seat, learner = synthetic()
    batches = learner.minibatches(sink, B, generator=torch.Generator(device="cuda").manual_seed(5))
    count = len(batches)
    if what == "fused-eager":
        fn = lambda: [learner.update(sink, b) for b in batches]  # noqa: E731
    elif what == "fused-graph":
        learner.update(sink, batches[0])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for b in batches:
                learner.update(sink, b)
        fn = graph.replay
    else:
        step = TorchUpdate(pol, seat)
        fn = lambda: [step(sink, b) for b in batches]  # noqa: E731
    (g, glo, ghi), (w, wlo, whi) = timed(fn)
    print("B=%d %s, %d updates per epoch: GPU %.1f us/update (%.1f .. %.1f), wall %.1f us/update (%.1f .. %.1f)"
          % (B, what, count, g / count * 1e6, glo / count * 1e6, ghi / count * 1e6, w / count * 1e6, wlo / count * 1e6,
             whi / count * 1e6), flush=True)
    print("RESULT %s %d %.6e %.6e" % (what, B, g / count, w / count), flush=True)


def round_trip(what, B):
    import torch
    from gym_comm_amd.vec_env import (FusedActorCriticPartner, MLPActorCritic, OvercookedVecEnv, PPOLearner,
                                      RolloutSink)
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500, ego_config={},
                          partner_config={}, num_communication=C, communication_on=True, ego_led=False, fow_radius=2)
    sink = RolloutSink(T, N, F, obs_dtype=torch.float32, fused=True)
    pol = MLPActorCritic(3, C, seed=1).cuda()
    seat = FusedActorCriticPartner(pol, sample=True, seed=3, sink=sink)
    venv = OvercookedVecEnv(arg, N, partner=seat, seed=1, obs_dtype=torch.float32)
    assert venv._b.F == F
    venv.reset_tensors()
    step = venv.closed_loop(None, graph=True, steps=16).step
    learner = PPOLearner(seat, **HP)
    torch_step = TorchUpdate(pol, seat)

    def one_round():
        sink.reset()
        for _ in range(T // 16):
            step()
        seat.finish_rollout()
        if what == "round-fused":
            learner.train(sink, n_epochs=10, batch_size=B)
        else:
            assert sink.full()
            for _ in range(10):
                for b in learner.minibatches(sink, B):
                    torch_step(sink, b)
    (g, glo, ghi), (w, wlo, whi) = timed(one_round, blocks=5)
    print("%s: collect %d x %d, GAE, 10 epochs at B=%d: wall %.2f ms (%.2f .. %.2f), GPU %.2f ms"
          % (what, T, N, B, w * 1e3, wlo * 1e3, whi * 1e3, g * 1e3), flush=True)
    print("RESULT %s %d %.6e %.6e" % (what, B, g, w), flush=True)


def one(what, B):
    import torch
    assert torch.cuda.is_available(), "ppo_update_rates.py measures on a GPU"
    (round_trip if what.startswith("round") else updates)(what, B)


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
                got[(what, B)] = (float(line.split()[3]), float(line.split()[4]))
            else:
                print(line, flush=True)
        if r.returncode != 0:
            sys.exit("measurement %s B=%d ended with status %d: stopping" % (what, B, r.returncode))
        if what == "torch":
            t, e, g = got[("torch", B)], got[("fused-eager", B)], got[("fused-graph", B)]
            print("B=%d     -> wall: torch %.1f us, fused eager %.1f us (%.1fx); GPU: torch %.1f us, fused captured %.1f us (%.1fx)"
                  % (B, t[1] * 1e6, e[1] * 1e6, t[1] / e[1], t[0] * 1e6, g[0] * 1e6, t[0] / g[0]), flush=True)
        if what == "round-torch":
            a, b = got[("round-torch", B)], got[("round-fused", B)]
            print("        -> a round: torch update %.2f ms, fused update %.2f ms (%.1fx)" % (a[1] * 1e3, b[1] * 1e3, a[1] / b[1]),
                  flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]))
    else:
        main()
