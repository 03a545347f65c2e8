#!/usr/bin/env python3
"""A learner in the partner seat on one MI355X, without a torch launch on the hot path: the seat acts,
records and steps inside a captured hipGraph (`FusedActorCriticPartner` + a fused `RolloutSink`), GAE
is one launch, and every minibatch of the PPO update is three (`PPOLearner`, include/oc_policy.h:
`oc_policy_ppo_update`).  The ego plays at random.  With --graph a whole train() -- the shuffle, every
minibatch, the KL stop -- is ONE more graph (`PPOLearner.train_graph`), and the round's statistics are
the means over its updates (`train_stats`).

    python examples/train_ppo.py --envs 4096 --rounds 20
    python examples/train_ppo.py --envs 4096 --rounds 20 --graph --target-kl 0.03
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gym_comm_amd.arglist import load_env_args
from gym_comm_amd.vec_env import (FusedActorCriticPartner, MLPActorCritic, OvercookedVecEnv, PPOLearner,
                                  RandomPartner, RolloutSink)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--level", default="open-divider_tomato")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--n-steps", type=int, default=128)
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--batch-size", type=int, default=16384)
    p.add_argument("--graph", action="store_true", help="train() as one captured graph (device shuffle)")
    p.add_argument("--clip-range-vf", type=float, default=None)
    p.add_argument("--target-kl", type=float, default=None, help="stop a train() early (with --graph)")
    a = p.parse_args()
    C = 2
    cfg = load_env_args({"level": a.level, "num_agents": 2, "max_num_timesteps": 100,
                         "communication_on": True, "num_communication": C, "fow_radius": 2})
    venv = OvercookedVecEnv(cfg, a.envs, obs_dtype=torch.float32)
    sink = RolloutSink(a.n_steps, a.envs, venv._b.F, obs_dtype=torch.float32, fused=True)
    pol = MLPActorCritic(venv._b.S, C, seed=0).cuda()
    venv.partner = seat = FusedActorCriticPartner(pol, sample=True, seed=1, sink=sink)
    learner = PPOLearner(seat, lr=3e-4, ent_coef=0.01, clip_range_vf=a.clip_range_vf, target_kl=a.target_kl)
    train = None                                                      # captured after the first rollout
    venv.reset_tensors()
    per = 16 if a.n_steps % 16 == 0 else 1
    loop = venv.closed_loop(RandomPartner(C, seed=2), steps=per)      # ego -> seat (act, record) -> step, per replay
    for k in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.n_steps // per):                             # collect
            loop.step()
        seat.finish_rollout()                                         # GAE: one launch
        if a.graph:
            train = train or learner.train_graph(sink, a.epochs, batch_size=a.batch_size, seed=k)
            train.replay()
        else:
            learner.train(sink, n_epochs=a.epochs, batch_size=a.batch_size)
        sink.reset()
        st = learner.stats()                                          # the round's only synchronisation
        if a.graph:
            ts = learner.train_stats()                                # (and this one: means over the round's updates)
            st.update({k_: ts[k_] for k_ in ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")})
        dt = time.perf_counter() - t0
        m = venv.metrics()
        print("round %3d  %.1f ms  loss %.4f  policy %.4f  value %.4f  entropy %.3f  kl %.4f  clipped %.2f  |g| %.3f  "
              "episodes %d  reward_sum %d" % (k, dt * 1e3, st["loss"], st["policy_loss"], st["value_loss"],
                                              -st["entropy_loss"], st["approx_kl"], st["clip_fraction"], st["grad_norm"],
                                              m["episodes"], m["reward_sum"])
              + ("  updates %d%s" % (ts["updates"], " (KL stop)" if ts["stopped"] else "") if a.graph else ""))


if __name__ == "__main__":
    main()
