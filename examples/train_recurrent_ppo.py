#!/usr/bin/env python3
"""A recurrent learner that learns, on one MI355X: an LSTM actor-critic (64 units) in the partner's seat, one
launch per step (`oc_policy_lstm_ac`), recording into a fused `RolloutSink` from a closed loop captured as one
hipGraph per 16 steps; then GAE in one launch and the PPO update over whole recorded sequences --
backpropagation through time, clip, Adam and the repack of the seat's weights -- in six launches per minibatch
(`RecurrentPPOLearner`, include/oc_policy.h: `oc_policy_rppo_update`).  With `--graph` the whole train() -- the
epochs' shuffles of the envs, the minibatches, the KL stop, value clipping, the logged means -- is ONE captured
graph (`train_graph`, `oc_policy_recurrent_train_step`), replayed once per round.  With `--window W` the seat records
its state every W steps (`RolloutSink(state_window=W)`, `oc_policy_window_snapshot`) and a minibatch is a set of
WINDOWS of W steps, each unrolled from its recorded state (`train_windows`, `oc_policy_window_gather`): truncated
backpropagation through time.

    python examples/train_recurrent_ppo.py --envs 4096 --rounds 4
    python examples/train_recurrent_ppo.py --envs 4096 --rounds 4 --graph --target-kl 0.03 --clip-range-vf 0.2
    python examples/train_recurrent_ppo.py --envs 4096 --rounds 4 --graph --window 16 --sequences-per-batch 8192
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gym_comm_amd.arglist import load_env_args
from gym_comm_amd.vec_env import (FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RecurrentPPOLearner,
                                  RolloutSink)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--level", default="open-divider_tomato")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--n-steps", type=int, default=128)
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--envs-per-batch", type=int, default=1024)
    p.add_argument("--window", type=int, default=None, help="train on windows of this many steps (it divides --n-steps)")
    p.add_argument("--sequences-per-batch", type=int, default=None,
                   help="with --window: windows per minibatch (default: --envs-per-batch x n-steps / window, the same samples)")
    p.add_argument("--graph", action="store_true", help="replay one captured train_graph per round; print train_stats()")
    p.add_argument("--target-kl", type=float, default=None, help="no epoch after one whose mean approx_kl exceeds 1.5 x this")
    p.add_argument("--clip-range-vf", type=float, default=None, help="value clipping around the recorded value")
    a = p.parse_args()
    if a.n_steps % 16:
        p.error("--n-steps is a multiple of 16 (the closed loop replays 16 steps at a time)")
    if a.window is not None and (a.window < 1 or a.n_steps % a.window):
        p.error("--window divides --n-steps")
    per = a.sequences_per_batch or (a.envs_per_batch * a.n_steps // a.window if a.window else None)
    C = 2
    cfg = load_env_args({"level": a.level, "num_agents": 2, "max_num_timesteps": 100,
                         "communication_on": True, "num_communication": C, "fow_radius": 2})
    venv = OvercookedVecEnv(cfg, a.envs, obs_dtype=torch.float32)
    pol = LSTMActorCritic(venv._b.S, C, seed=1).cuda()
    sink = RolloutSink(a.n_steps, a.envs, venv._b.F, obs_dtype=torch.float32, fused=True, state_window=a.window)
    venv.partner = seat = FusedRecurrentPartner(pol, sample=True, seed=7, sink=sink)
    learner = RecurrentPPOLearner(seat, lr=3e-4, ent_coef=0.01, clip_range_vf=a.clip_range_vf, target_kl=a.target_kl)
    device = a.graph or a.target_kl is not None or a.clip_range_vf is not None    # both live in the train sequence
    graph = None
    venv.reset_tensors()
    loop = venv.closed_loop(None, steps=16)          # the ego's action rows stay as they are (all zeros)
    for r in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seat.begin_rollout(a.envs)                   # the state this rollout starts from; the sink reset
        for _ in range(a.n_steps // 16):
            loop.step()
        seat.finish_rollout(gamma=0.99, gae_lambda=0.95)
        if a.graph:
            if graph is None:                        # the first full, finished sink: checked here, captured once
                graph = (learner.train_graph_windows(sink, a.epochs, sequences_per_batch=per, seed=r) if a.window else
                         learner.train_graph(sink, a.epochs, envs_per_batch=a.envs_per_batch, seed=r))
            graph.replay()
        elif a.window:
            learner.train_windows(sink, n_epochs=a.epochs, sequences_per_batch=per, shuffle="device" if device else "torch",
                                  seed=r)
        else:
            learner.train(sink, n_epochs=a.epochs, envs_per_batch=a.envs_per_batch, shuffle="device" if device else "torch",
                          seed=r)
        stats = learner.stats()                      # the round's one synchronisation
        dt = time.perf_counter() - t0
        if device:
            ts = learner.train_stats()
            print("round %d: train_stats: %d updates in %d epochs%s; means: loss %.4f policy %.4f value %.4f entropy %.4f "
                  "kl %.5f clip %.3f" % (r, ts["updates"], ts["epochs"], " (stopped by target_kl)" if ts["stopped"] else "",
                                         ts["loss"], ts["policy_loss"], ts["value_loss"], ts["entropy_loss"], ts["approx_kl"],
                                         ts["clip_fraction"]))
        print("round %d: %.1f ms; mean reward %.4f; last minibatch: loss %.4f policy %.4f value %.4f entropy %.4f "
              "kl %.5f clip %.3f |g| %.3f bad %d"
              % (r, dt * 1e3, sink.rewards.mean().item(), stats["loss"], stats["policy_loss"], stats["value_loss"],
                 stats["entropy_loss"], stats["approx_kl"], stats["clip_fraction"], stats["grad_norm"], int(stats["bad"])))


if __name__ == "__main__":
    main()
