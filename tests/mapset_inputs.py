"""Inputs shared by test_mapset_structures_gpu.py and test_mapset_structures_cpu.py -- not a test module,
and nothing here touches a device.  (`actions` and `reference` take `_inputs` and `SetOracle` from
test_mapset_gpu.py, where the first map-set cases keep them; that module imports torch and runs nothing
on import, so the CPU test can use them.)

The GPU cases step map sets of the shipped random-* Salad family, of a pair of maps that repeat a type,
of Salad maps with a time limit each and of the tl maps, against one oracle per map (test_mapset_gpu.py:
SetOracle); the CPU test checks with the oracle alone that these inputs reach what the cases are about.
Every case is a row of CASES: its maps, the group -> map assignment, n, the step count and where the
items of a random-* map start.  `reference(case)` is the oracles' run of a case whose
placements are known ahead (every one but the in-kernel draw), computed once and shared read-only.
"""
import functools
import os

import numpy as np

from conftest import GOLDEN, load_golden

SEED = 23
# the eight shipped random-*_salad levels, by Counter count; one structure, one subtask order
SALAD8 = ["random-open-divider_salad_small",            # 5 x 5,  9 Counters
          "random-open-divider_salad_small_cramped",    # 6 x 5, 14, agent 0 starts in the (0, 0) corner
          "random-open-divider_salad",                  # 7 x 7, 17
          "random-salad-superwide",                     # 11 x 4, 19
          "random-partial-divider_salad",               # 7 x 7, 20
          "random-full-divider_salad",                  # 7 x 7, 20
          "random-open-divider_salad_small_wide",       # 9 x 5, 23
          "random-open-divider_salad_small_wide_big"]   # 8 x 7, 29
CRAMPED = SALAD8[1]
FAMILY = [m for m in SALAD8 if m != CRAMPED]
RANDOM_TOMATO = ["random-open-divider_tomato", "random-full-divider_tomato"]
SALAD = ["open-divider_salad", "partial-divider_salad", "full-divider_salad"]
TL = ["open-divider_tl", "partial-divider_tl", "full-divider_tl"]
TL_ORDER = [3, 0, 4, 1, 2, 5]           # a caller's order of the six tl subtasks; the two Deliver subtasks (2, 5)
                                        # keep their relative order, which the structure library folds in

# custom-two_tomatoes (tests/golden/cbase_dup_two_tomatoes_a2.npz) with another interior: a divider
# column with two gaps, the Delivery tile on the south wall, one tomato on the west wall
DUP_VARIANT = ("--t----\n/  -  l\n/  -  -\nt     -\n-  -  -\n-     p\n---*-p-\n\nSimpleTomato\n\n"
               "2 1\n4 1\n4 4\n2 4")
# what agent 0 of every third env plays from every time limit on (D U L R = 0 1 2 3): both tomatoes
# to the two Cutboards, then one chopped tomato onto the other
DUP_SCRIPTS = ("LULRRRRULLLLDLULDL",        # custom-two_tomatoes: (1, 0) and (5, 0) -> (0, 1) and (0, 2)
               "ULLDDLULULDL")              # the variant: (2, 0) and (0, 3) -> (0, 1) and (0, 2)
_CODE = {"D": 0, "U": 1, "L": 2, "R": 3}

# name: (maps, T per map, group -> map, n, steps, placement)
#   placement: None (no scattered items), "nominal" (each map's own nominal cells, what the constructor
#   of placement_mode="host" starts on), "pattern" (host_cells(k) before every step) or "rng" (the
#   in-kernel draw: the GPU case reads it back; the CPU twin runs "pattern" in its place)
CASES = {
    # nine groups on seven maps, none sorted; the 37-env group lives on a map of 20 Counters
    "family": (tuple(FAMILY), (25,) * 7, (3, 0, 6, 1, 5, 2, 4, 0, 3), 8 * 64 + 37, 120, "rng"),
    "host": (tuple(FAMILY[i] for i in (0, 5, 2, 6)), (25,) * 4, (0, 1, 2, 3), 229, 60, "pattern"),
    "cramped": ((FAMILY[0], CRAMPED, FAMILY[5]), (25,) * 3, (0, 1, 2), 165, 120, "nominal"),
    "dup": (("custom-two_tomatoes", "two_tomatoes-variant"), (30, 30), (0, 1, 1, 0), 229, 120, None),
    "per-map-T": (tuple(SALAD), (12, 25, 40), (0, 1, 2, 1), 229, 120, None),
    "tl": (tuple(TL), (25,) * 3, (2, 0, 1, 0), 229, 120, None),
    "vec-env": (tuple(FAMILY[i] for i in (1, 0, 6)), (25,) * 3, (0, 1, 2), 165, 30, "rng"),
}


STAGGER = {4: 1, 8: 2}          # after step k: the envs of map 1 with i % 3 == STAGGER[k] are reset by hand


def stagger_mask(case, k):
    """int32 [n] mask of a reset by hand after step k, or None.  The time limits 12, 25 and 40 alone end
    episodes on 16 of 120 steps.  On the T = 25 map (two groups, one of them partial) a third of the envs
    starts over after step 4 and another third after step 8 -- 5 and 9 steps behind their map from then
    on, which still leaves them four whole episodes -- and the done row is mixed on 23."""
    if case != "per-map-T" or k not in STAGGER:
        return None
    return ((env_map(case) == 1) & (np.arange(CASES[case][3]) % 3 == STAGGER[k])).astype(np.int32)


def golden_level_text(fixture):
    _, st = load_golden(os.path.join(GOLDEN, fixture))
    return st["level"], st["level_text"]


@functools.lru_cache(maxsize=None)
def compiled(name, T, order=None):
    from gym_comm_amd import compiler, levels
    if name == "custom-two_tomatoes":
        name = levels.parse_level_text(*golden_level_text("cbase_dup_two_tomatoes_a2.npz"))
    elif name == "custom-two_tomatoes_small":
        name = levels.parse_level_text(*golden_level_text("cbase_dup_two_tomatoes_small_a2.npz"))
    elif name == "two_tomatoes-variant":
        name = levels.parse_level_text("two_tomatoes-variant", DUP_VARIANT)
    return compiler.compile_level(name, 2, T, subtask_order=None if order is None else list(order))


def case_levels(case):
    names, Ts = CASES[case][:2]
    order = tuple(TL_ORDER) if case == "tl" else None
    return [compiled(m, T, order) for m, T in zip(names, Ts)]


def env_map(case):
    """The map index of every env."""
    _, _, gm, n, _, _ = CASES[case]
    return np.asarray(gm)[np.arange(n) // 64]


def counter_cells(lv):
    return np.array([x | (y << 4) for x, y in lv.counters], np.int32)


def host_cells(case, k):
    """int32 [M][n] start cells of a set of random-* maps: the scattered item j of env i goes to Counter
    (o + j) mod c of ITS map (c Counters, at least 9, so an env's cells are distinct).  k = -1: o = 3 i,
    the cells of the first reset; k >= 0: o seeded by k, the cells an env that finishes at step k takes."""
    n = CASES[case][3]
    lvs = case_levels(case)
    out = nominal_cells(case)
    off = 3 * np.arange(n) if k < 0 else np.random.default_rng(1000 * SEED + k).integers(0, 1 << 16, n)
    em = env_map(case)
    for m, lv in enumerate(lvs):
        cc, ix = counter_cells(lv), np.nonzero(em == m)[0]
        for j, item in enumerate(lv.scatter_items):
            out[item, ix] = cc[(off[ix] + j) % len(cc)]
    return out


@functools.lru_cache(maxsize=None)
def actions(case):
    """(actions [steps][4][n] int32, the in-kernel partner's stream words [steps + 1][n]): the seeded
    momentum stream of test_mapset_gpu.py (seed 23, keep 0.6) with the partner's own draw as its rows."""
    from test_mapset_gpu import _inputs
    _, Ts, _, n, steps, _ = CASES[case]
    acts, words = _inputs(n, 120)
    acts, words = acts[:steps], words[:steps + 1]
    if case == "dup":       # every third env's agent 0 walks to the tomatoes, episode after episode
        acts = acts.copy()
        em, T = env_map(case), Ts[0]
        for m, script in enumerate(DUP_SCRIPTS):
            ix = np.nonzero((em == m) & (np.arange(n) % 3 == 0))[0]
            for k in range(steps):
                if k % T < len(script):
                    acts[k, 0, ix] = _CODE[script[k % T]]
        acts.setflags(write=False)
    return acts, words


@functools.lru_cache(maxsize=None)
def reference(case):
    """Every step of the case under SetOracle (one oracle per map), read-only.  Maps that scatter items
    step with auto_reset off and re-place the envs that finished on the case's own cells."""
    from test_mapset_gpu import SetOracle
    _, _, gm, n, steps, placement = CASES[case]
    acts, _ = actions(case)
    ora = SetOracle(case_levels(case), gm, n)
    moving = placement in ("pattern", "rng")
    if placement is not None:
        ora.set_placement(host_cells(case, -1) if moving else nominal_cells(case))
    ora.reset()
    out = [{"snapshot": ora.snapshot()}]            # [0]: after the reset; [k + 1]: after step k
    for k in range(steps):
        if moving:
            r = ora.replace_finished(ora.multi_step(acts[k], auto_reset=False), host_cells(case, k))
        else:
            r = ora.multi_step(acts[k])
        out.append(r)
        if stagger_mask(case, k) is not None:
            ora.reset(stagger_mask(case, k))
    for r in out:
        for v in list(r.values()) + list(r["snapshot"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def nominal_cells(case):
    """int32 [M][n]: every env on the cells its own map was compiled with (a random-* map: its first Counters)."""
    cols = np.array([[x | (y << 4) for _, x, y in lv.items] for lv in case_levels(case)], np.int32)
    return np.ascontiguousarray(cols[env_map(case)].T)
