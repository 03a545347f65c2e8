#!/usr/bin/env python3
"""A recurrent learner in the partner's seat on one MI355X: an LSTM actor-critic (64 units) whose whole
step -- masked state, cell, both heads, the sampled action, its log-probability and the value -- is ONE
launch (`oc_policy_lstm_ac`, include/oc_policy.h), recording into a fused `RolloutSink`; partner -> fused
step -> update run as one hipGraph per 16 steps.  --policy torch runs the same module through
`RecurrentPolicyPartner` instead (some forty launches per step).

    python examples/recurrent_seat.py --envs 4096 --rollouts 4
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gym_comm_amd.arglist import load_env_args
from gym_comm_amd.vec_env import (FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RecurrentPolicyPartner,
                                  RolloutSink)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--level", default="open-divider_tomato")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--rollouts", type=int, default=4)
    p.add_argument("--n-steps", type=int, default=128)
    p.add_argument("--policy", default="fused", choices=["fused", "torch"])
    a = p.parse_args()
    C = 2
    cfg = load_env_args({"level": a.level, "num_agents": 2, "max_num_timesteps": 100,
                         "communication_on": True, "num_communication": C, "fow_radius": 2})
    venv = OvercookedVecEnv(cfg, a.envs, obs_dtype=torch.float32)
    pol = LSTMActorCritic(venv._b.S, C, seed=1).cuda()
    sink = RolloutSink(a.n_steps, a.envs, venv._b.F, obs_dtype=torch.float32, fused=True)
    if a.policy == "fused":
        venv.partner = seat = FusedRecurrentPartner(pol, sample=True, seed=7, sink=sink)
    else:       # the module puts the zero state into starting envs itself
        venv.partner = seat = RecurrentPolicyPartner(pol, pol.initial_state(a.envs, "cuda"), sample=True, seed=7,
                                                     sink=sink, mask_state=False)
    venv.reset_tensors()
    loop = venv.closed_loop(None, steps=16)          # the ego's action rows stay as they are (all zeros)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(a.rollouts):
        for _ in range(a.n_steps // 16):
            loop.step()
        adv, ret = seat.finish_rollout(gamma=0.99, gae_lambda=0.95)      # [n_steps][n]; a recurrent update goes here
        sink.reset()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = a.rollouts * (a.n_steps // 16) * 16
    print("%d envs x %d steps (%s seat): %.1f us/step; last rollout: mean value %.4f, mean return %.4f, %d episode starts"
          % (a.envs, steps, a.policy, dt / steps * 1e6, sink.values.mean().item(), ret.mean().item(),
             int(sink.episode_starts.sum().item())))


if __name__ == "__main__":
    main()
