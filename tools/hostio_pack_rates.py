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
from gym_comm_amd import _lib
from gym_comm_amd.vec_env import MappedBuffer, OvercookedVecEnv


def main():
    for n in (4096, 131072):
        arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=500,
                              ego_config={}, partner_config={}, num_communication=2,
                              communication_on=True, ego_led=False, fow_radius=2)
        venv = OvercookedVecEnv(arg, n, seed=1)
        venv.reset_tensors()
        b, hp = venv._b, venv._host_plan()
        L, w = hp["L"], hp["width"]
        total = hp["dev"].numel()
        mapped = MappedBuffer(L, b._dev_index, total)

        def pack(name, out):
            _lib.call(L, name, b._dev_index, b.obs[0].data_ptr(), hp["ot"], b.F, hp["plan"].data_ptr(), w[0], w[1], w[2],
                      b.timestep.data_ptr(), b.shaped_reward.data_ptr(), b.ep_return.data_ptr(), b.done.data_ptr(),
                      b.ep_length.data_ptr(), out, n)

        dev = hp["dev"].data_ptr()
        rows = [("oc_pack_host -> device", lambda: pack("oc_pack_host", dev)),
                ("oc_pack_host_tiled -> device", lambda: pack("oc_pack_host_tiled", dev)),
                ("oc_pack_host_tiled -> host-mapped", lambda: pack("oc_pack_host_tiled", mapped.dev))]
        for rnd in (1, 2):
            out = ["n = %d, %d bytes per step, pass %d:" % (n, total, rnd)]
            for label, fn in rows:
                us = timed(fn)
                out.append("%s %.2f us (%.1f GB/s)" % (label, us, total / us * 1e-3))
            print("  ".join(out), flush=True)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
