#!/usr/bin/env python3
"""Per-launch time of the numpy boundary's two pack kernels (include/oc_hostio.h) on a real step's
rows: oc_pack_host and oc_pack_host_tiled into a device buffer, and oc_pack_host_tiled into a
host-mapped buffer (its stores cross PCIe) -- hipGraph replays of 64 launches, HIP events.
GPU box only."""
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from aux_kernel_rates import timed
from gym_comm_amd.hostio import HostCopy, MappedBuffer
from gym_comm_amd.vec_env import OvercookedVecEnv


def main():
    for n in (4096, 131072):
        arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500,
                              ego_config={}, partner_config={}, num_communication=2,
                              communication_on=True, ego_led=False, fow_radius=2)
        venv = OvercookedVecEnv(arg, n, seed=1)
        venv.reset_tensors()
        io = HostCopy(venv)             # the env's own plan and pack launch (episode statistics on)
        total = io.plan.total
        mapped = MappedBuffer(io.L, venv._b._dev_index, total)
        dev = io.dev.data_ptr()
        rows = [("oc_pack_host -> device", lambda: io.pack("oc_pack_host", dev)),
                ("oc_pack_host_tiled -> device", lambda: io.pack("oc_pack_host_tiled", dev)),
                ("oc_pack_host_tiled -> host-mapped", lambda: io.pack("oc_pack_host_tiled", mapped.dev))]
        for rnd in (1, 2):
            out = ["n = %d, %d bytes per step, pass %d:" % (n, total, rnd)]
            for label, fn in rows:
                us = timed(fn)
                out.append("%s %.2f us (%.1f GB/s)" % (label, us, total / us * 1e-3))
            print("  ".join(out), flush=True)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
