"""Maps above 64 cells for tests/test_big_maps_cpu.py and tests/test_big_maps_gpu.py: the maps, seeded
inputs that really reach the far columns and rows, and the oracle's results of every step, computed
once per (map, agents, kind) and shared read-only.

The recorded maps come out of their fixtures (tests/golden, `level_text`), so the seeded runs step the
maps the reference itself was run on; three more are written here."""
import functools
import os

import numpy as np

from conftest import GOLDEN, load_golden
from hip_util import momentum_actions

# name -> fixture that carries the level text
RECORDED = {"wide_16x8": "cbase_custom-big_wide_salad_a2.npz",        # 128 cells, W = 16 (dense() multiplier 0)
            "tall_8x16": "cbase_custom-big_tall_salad_a3.npz",        # 128 cells, rows up to 15
            "odd_13x9": "cbase_custom-big_odd_tomato_a4.npz",         # 117 cells, an odd W
            "square_11x11": "fow_bigsquare_r3.npz",                   # 121 cells
            "dup_16x8": "cbase_dup_big_two_tomatoes_a2.npz",          # a repeated type: the per-cell probe table
            "random_16x8": "rbase_random-big_salad_a2.npz"}           # 49 Counters, four scattered items
WRITTEN = {
    # 64 cells: the largest map whose tile planes fit one word (the other side of `nc > 64`)
    "control_8x8": "-t----l-\n/      -\n/      -\n*  --  -\n-      -\n-      p\n-      p\n--------\n\nSalad\n\n2 1\n5 5\n3 4",
    # 120 cells with the 16 x 8 map's structure (Salad; Tomato, Lettuce, two Plates in scan order; a
    # closed border): its partner in a map set
    "variant_12x10": "-t----l-----\n/          -\n/    --    -\n-          -\n*          -\n-   ----   p\n-          p\n"
                     "-          -\n-          -\n------------\n\nSalad\n\n2 1\n9 8\n6 4",
}
MAPS = dict(RECORDED, **WRITTEN)
N, STEPS, T, SEED = 229, 120, 30, 31        # a 37-env last group; every env auto-resets four times


@functools.lru_cache(maxsize=None)
def level_text(name):
    if name in WRITTEN:
        return WRITTEN[name]
    return load_golden(os.path.join(GOLDEN, RECORDED[name]))[1]["level_text"]


@functools.lru_cache(maxsize=None)
def level(name, agents, t=T):
    from gym_comm_amd import compiler, levels
    return compiler.compile_level(levels.parse_level_text("big-" + name, level_text(name)), agents, t)


# what agent 0 plays from its start (2, 1) to reach the far side (action codes: 0 = +y, 2 = -x, 3 = +x)
WALK = {"wide_16x8": [3] * 12, "dup_16x8": [3] * 12, "random_16x8": [3] * 12,      # along row 1 to x = 14
        "tall_8x16": [2] + [0] * 13,                                               # down column 1 to y = 14
        "odd_13x9": [3] * 9, "square_11x11": [3] * 7, "variant_12x10": [3] * 8, "control_8x8": [3] * 4}


@functools.lru_cache(maxsize=None)
def moves(name, agents, nact, n=N, steps=STEPS):
    """[steps][agents][n] action codes below `nact`: momentum-random, and in every third env agent 0
    first walks to the far side of the map (the other agents stay random, so some walks are blocked)."""
    rng = np.random.default_rng(SEED + agents)
    acts = momentum_actions(rng, steps, agents, n, keep=0.6, nact=nact)
    walk = WALK[name]
    for k, a in enumerate(walk):
        acts[k, 0, ::3] = a
    acts.setflags(write=False)
    return acts


def far_reached(name, snapshots):
    """From the oracle's snapshots: some env has an agent in the last floor column / row the walk heads for."""
    lv = level(name, 2)
    axis, want = (1, lv.height - 2) if name == "tall_8x16" else (0, lv.width - 2)
    return any((s["agents"][:, :, axis] >= want).any() for s in snapshots)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


@functools.lru_cache(maxsize=None)
def base_reference(name, agents, placement=None):
    """The oracle's base step over moves(name, agents, 5): per step reward, done, shaping, snapshot."""
    from oracle import oracle
    lv = level(name, agents)
    acts = moves(name, agents, 5)
    ora = oracle.OracleBatch(lv.blob, N, threads=4)
    if placement is not None:
        ora.set_placement(np.frombuffer(placement, np.int32).reshape(lv.num_items, N))
        ora.reset()
    out = []
    for k in range(STEPS):
        r, d, sh = ora.step(acts[k], auto_reset=True)
        out.append(_freeze({"reward": r, "done": d, "shaping": sh, "snapshot": ora.snapshot_all()}))
    assert all((s["snapshot"]["error"] == 0).all() for s in out)         # no env-step is excluded
    assert min(sum(int(s["done"][i]) for s in out) for i in range(N)) >= STEPS // T
    assert sum(int(s["reward"].sum()) for s in out) > 0
    assert far_reached(name, [s["snapshot"] for s in out])
    return out


def fused_actions(name, C, n=N, steps=STEPS):
    mv = moves(name, 2, 4, n, steps)
    cm = np.random.default_rng(SEED + 100 + C).integers(0, C, (steps, 2, n))
    return np.stack([mv[:, 0], cm[:, 0], mv[:, 1], cm[:, 1]], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def fused_reference(name, C, radius, blind=0):
    """The oracle's wrapper step (2 agents) over fused_actions(name, C): per step both viewers' rows,
    timestep, shaped reward, done, comm, sparse reward and the snapshot."""
    from oracle import oracle
    lv = level(name, 2)
    acts = fused_actions(name, C)
    ora = oracle.OracleBatch(lv.blob, N, threads=4)
    comm = np.zeros((2, N), np.int32)
    out = []
    for k in range(STEPS):
        o, ts, r, d = ora.multi_step(acts[k], comm, radius, blind, C, auto_reset=True)
        out.append(_freeze({"obs": o, "timestep": ts, "reward": r, "done": d, "comm": comm.copy(),
                            "sparse": ora.last_step()["sparse"].copy(), "snapshot": ora.snapshot_all()}))
    assert all((s["snapshot"]["error"] == 0).all() for s in out)
    assert min(sum(int(s["done"][i]) for s in out) for i in range(N)) >= STEPS // T
    assert far_reached(name, [s["snapshot"] for s in out])
    return out
