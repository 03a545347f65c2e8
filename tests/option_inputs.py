"""Inputs and plain restatements shared by test_multi_step_options_gpu.py, test_obs_image_gpu.py and
test_option_inputs_cpu.py -- not a test module.

The GPU tests compare the fused step's general variant and the image kernel with the oracle on the
inputs built here; the CPU test checks, with the oracle alone, that these inputs reach what the GPU
cases are about (episodes that end, a batch out of lockstep, held / chopped / merged objects), so
that no GPU case can pass vacuously.

Restated here, from the headers' definitions and not from the kernels:

  partner_draw     the in-kernel partner (include/oc_hip.h, oc_step_opts.alt_rng): two PCG32 steps
                   per env per step, move = umulhi(out, 4), comm = umulhi(out, C)
  stats_step       the episode statistics (ep_return / ep_length): numpy fp64, one addition
"""
import functools
import os

import numpy as np

from conftest import GOLDEN, load_golden
from hip_util import momentum_actions, scripted_then_random
from policy_ref import pcg32

# ---- the fused step's options ------------------------------------------------------------------
STEPS, T, C, RADIUS, NMAX = 60, 12, 3, 1, 130
SEED = 7
SNAP_EVERY = 10
STAGGER = 6                      # after step k < STAGGER the envs with i % 7 == k + 1 are reset

_P = {"BLIND": False, "CAN_MOVE": True}
# every wrapper configuration is non-standard on at least one axis; together they flip every axis
CONFIGS = {
    "ego-led": dict(ego_led=True),
    "comm-off": dict(communication_on=False),
    "ego-is-1": dict(ego_agent_idx=1),
    "blind-ego+partner-still": dict(ego=dict(_P, BLIND=True), partner=dict(_P, CAN_MOVE=False)),
    "all-flipped": dict(ego_led=True, ego_agent_idx=1, ego=dict(_P, CAN_MOVE=False), partner=dict(_P, BLIND=True)),
    "play": dict(play=True),
}
MULTI_LEVELS = ["full-divider_salad", "open-divider_tomato", "random-open-divider_salad_small"]
RNG_LEVEL = "random-open-divider_salad_small"        # stepped with placement_mode="rng"


def config(cfg_id):
    """The full configuration of an id of CONFIGS: wrapper keywords, masks and the play flag."""
    c = dict(communication_on=True, ego_led=False, ego_agent_idx=0, ego=dict(_P), partner=dict(_P), play=False)
    c.update(CONFIGS[cfg_id])
    c["blind_mask"] = (1 if c["ego"]["BLIND"] else 0) | (2 if c["partner"]["BLIND"] else 0)
    c["can_move_mask"] = (1 if c["ego"]["CAN_MOVE"] else 0) | (2 if c["partner"]["CAN_MOVE"] else 0)
    return c


def oracle_kw(cfg):
    return dict(communication_on=cfg["communication_on"], ego_led=cfg["ego_led"],
                ego_agent_idx=cfg["ego_agent_idx"], can_move_mask=cfg["can_move_mask"])


@functools.lru_cache(maxsize=None)
def multi_level(level, play=False):
    from gym_comm_amd import compiler
    return compiler.compile_level(level, 2, T, play=play)


def umulhi(a, b):
    return (np.asarray(a, np.uint64) * np.uint64(b)) >> np.uint64(32)


def partner_draw(state, num_comm):
    """One step of the in-kernel partner: (advanced stream words uint64 < 2^32, move, comm)."""
    s, o1 = pcg32(state)
    s, o2 = pcg32(s)
    return s, umulhi(o1, 4).astype(np.int32), umulhi(o2, num_comm).astype(np.int32)


@functools.lru_cache(maxsize=None)
def partner_stream():
    """The partner's seeded streams and what they draw: words [STEPS + 1][NMAX] as int32 bit patterns
    (row k = before step k), moves and comms [STEPS][NMAX]."""
    from gym_comm_amd.batched import pcg32_seed_states
    s = pcg32_seed_states(SEED, (NMAX,)).numpy().astype(np.int64).astype(np.uint64)
    words, mv, cm = [s], [], []
    for _ in range(STEPS):
        s, m, c = partner_draw(s, C)
        words.append(s), mv.append(m), cm.append(c)
    words = np.stack(words).astype(np.uint32).view(np.int32)
    out = (words, np.stack(mv), np.stack(cm))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def multi_actions(invalid=False):
    """[STEPS][4][NMAX] int64: ego move, ego comm (seeded; the moves keep their direction for a
    while), partner move, partner comm (the partner's draw itself, so that one oracle run serves the
    rows, the pairs and the in-kernel partner).  `invalid`: about 1 % invalid indices in
    every row (such a case takes both players from rows or pairs), among them two int64 values that do
    not fit int32; returned with a second array, what the oracle is given (any invalid int32, -1,
    for those two)."""
    rng = np.random.default_rng(SEED)
    mv = momentum_actions(rng, STEPS, 1, NMAX, keep=0.6, nact=4)[:, 0]
    cm = rng.integers(0, C, (STEPS, NMAX))
    _, pmv, pcm = partner_stream()
    acts = np.stack([mv, cm, pmv, pcm], axis=1).astype(np.int64)
    if not invalid:
        acts.setflags(write=False)
        return acts
    big = [(1 << 32) + 1, -(1 << 40)]
    for row, bad in ((0, [5, 7, -1]), (1, [C, -2, 99]), (2, [5, 7, -1]), (3, [C, -2, 99])):
        hit = rng.random((STEPS, NMAX)) < 0.01
        acts[:, row] = np.where(hit, rng.choice(bad + big, size=hit.shape), acts[:, row])
    narrow = np.where((acts < -2 ** 31) | (acts >= 2 ** 31), -1, acts)
    acts.setflags(write=False), narrow.setflags(write=False)
    return acts, narrow


def stagger_mask(k, n):
    """int32 [n] reset mask applied after step k, or None."""
    if k >= STAGGER:
        return None
    return (np.arange(n) % 7 == k + 1).astype(np.int32)


def host_cells(lv, n, rng):
    """Per-env start cells [M][n] of a random-* level (distinct Counter tiles, drawn on the host)."""
    place = np.zeros((lv.num_items, n), np.int32)
    for i in range(n):
        pick = rng.choice(len(lv.counters), size=len(lv.scatter_items), replace=False)
        for k, item in enumerate(lv.scatter_items):
            x, y = lv.counters[pick[k]]
            place[item, i] = x | (y << 4)
    return place


class MultiReference:
    """The oracle stepped through the multi-step input of (level, configuration): `step(k)` returns
    what the oracle leaves after step k (auto-reset applied) and `reset(mask)` applies a staggered
    reset.  A level placed by the in-kernel generator cannot be known ahead: the caller passes the
    cells the library drew (`cells`: [M][n], read back from its state) to the constructor, to `step`
    (used by the envs that ended) and to `reset`."""

    def __init__(self, level, cfg_id, n=NMAX, narrow=None, cells=None):
        from oracle import oracle
        oracle.build()
        self.cfg = config(cfg_id)
        self.lv = multi_level(level, self.cfg["play"])
        self.n = n
        self.acts = np.ascontiguousarray((multi_actions() if narrow is None else narrow)[:, :, :n].astype(np.int32))
        self.ora = oracle.OracleBatch(self.lv.blob, n)
        self.placed = self.lv.random_placement
        if self.placed:
            self.ora.set_placement(cells)
            self.ora.reset()
        self.comm = np.zeros((2, n), np.int32)

    def step(self, k, cells=None):
        cfg, ora, n = self.cfg, self.ora, self.n
        o, t, r, d = ora.multi_step(self.acts[k], self.comm, RADIUS, cfg["blind_mask"], C,
                                    auto_reset=not self.placed, **oracle_kw(cfg))
        last = {key: v.copy() for key, v in ora.last_step().items()}
        if self.placed and d.any():      # the fresh episodes of the envs that ended, on the cells given
            ora.set_placement(cells)
            ora.reset(d)
            for i in np.nonzero(d)[0]:
                for v in range(2):
                    o[v, :, i], t[i] = ora.obs(int(i), v, RADIUS, bool((cfg["blind_mask"] >> v) & 1),
                                               bool(cfg["blind_mask"] & 1), C, self.comm[:, i])
        snap = ora.snapshot_all()
        return dict(obs=o, timestep=t, reward=r, done=d, comm=self.comm.copy(), error=snap["error"],
                    snapshot=snap, **last)

    def reset(self, mask, cells=None):
        if self.placed:
            self.ora.set_placement(cells)
        self.ora.reset(mask)


@functools.lru_cache(maxsize=None)
def multi_reference(level, cfg_id, invalid=False):
    """Every step of MultiReference at NMAX envs for a fixed level, computed once and never modified
    (envs are independent: a smaller batch is its first n envs).  For the level placed at random the
    cells are drawn on the host here -- a stand-in for the library's own draw that serves the CPU
    test's conditions only."""
    lv = multi_level(level, config(cfg_id)["play"])
    rng = np.random.default_rng(SEED + 1)
    draw = (lambda: host_cells(lv, NMAX, rng)) if lv.random_placement else (lambda: None)
    ref = MultiReference(level, cfg_id, NMAX, multi_actions(True)[1] if invalid else None, draw())
    steps = []
    for k in range(STEPS):
        steps.append(ref.step(k, draw()))
        mask = stagger_mask(k, NMAX)
        if mask is not None:
            ref.reset(mask, draw())
    for s in steps:
        for v in list(s.values()) + list(s["snapshot"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return steps


def stats_step(ret, length, prev_done, reward):
    """One step of the episode statistics in numpy fp64 (include/oc_hip.h: ep_return / ep_length)."""
    p = np.asarray(prev_done) != 0
    ret, reward = np.asarray(ret, np.float64), np.asarray(reward, np.float64)
    return np.where(p, reward, ret + reward), np.where(p, 1, np.asarray(length) + 1).astype(np.int32)


def stats_reference(rewards, dones):
    """Running (return [K][n] fp64, length [K][n] int32) over (reward, done) streams [K][n], from
    zeros and no previous done."""
    ret, length = np.zeros(rewards.shape[1]), np.zeros(rewards.shape[1], np.int32)
    prev = np.zeros(rewards.shape[1], np.int32)
    rets, lens = [], []
    for r, d in zip(rewards, dones):
        ret, length = stats_step(ret, length, prev, r)
        prev = d
        rets.append(ret), lens.append(length)
    return np.stack(rets), np.stack(lens)


# ---- the image observation -----------------------------------------------------------------------
IMG_N, IMG_STEPS, IMG_EVERY, IMG_T, IMG_SEED = 100, 120, 10, 45, 3
RADII = [0, 1, 2, 5, 1000]
# (level or dup fixture, agents, (W, H), merges required)
IMAGE_CASES = [
    ("open-divider_tl", 3, (7, 7), True),
    ("partial-divider_salad", 4, (7, 7), False),
    ("random-salad-superwide", 2, (11, 4), True),
    ("random-open-divider_salad_small_wide_big", 2, (8, 7), False),
    ("random-open-divider_salad_small", 2, (5, 5), True),
    ("cbase_dup_three_tomatoes_a3", 3, (7, 7), True),
    ("cbase_dup_two_lettuces_salad_a2", 2, (7, 7), True),
]
IMAGE_IDS = [c[0] for c in IMAGE_CASES]


@functools.lru_cache(maxsize=None)
def image_level(name, agents):
    from gym_comm_amd import compiler, levels
    if name.startswith("cbase_dup_"):
        _, st = load_golden(os.path.join(GOLDEN, name + ".npz"))
        return compiler.compile_level(levels.parse_level_text(st["level"], st["level_text"]), agents, IMG_T)
    return compiler.compile_level(name, agents, IMG_T)


@functools.lru_cache(maxsize=None)
def image_inputs(name, agents):
    """(actions [IMG_STEPS][A][IMG_N] int32, cells [M][IMG_N] or None): per-env action streams and,
    for a random-* level, per-env host placements."""
    lv = image_level(name, agents)
    rng = np.random.default_rng(IMG_SEED)
    cells = host_cells(lv, IMG_N, rng) if lv.random_placement else None
    if lv.has_dup:
        acts = momentum_actions(rng, IMG_STEPS, agents, IMG_N, keep=0.6)
    else:
        acts = scripted_then_random(rng, lv.name, IMG_STEPS, agents, IMG_N)
    acts = np.ascontiguousarray(acts.astype(np.int32))
    acts.setflags(write=False)
    return acts, cells


@functools.lru_cache(maxsize=None)
def image_reference(name, agents):
    """The oracle stepped through image_inputs with auto-reset; at every IMG_EVERY-th step the
    images and holding flags at every radius of RADII and the state snapshot.  Returns
    ({step: {"snapshot", radius: (maps, holding)}}, flagged env-steps)."""
    from oracle import oracle
    oracle.build()
    lv = image_level(name, agents)
    acts, cells = image_inputs(name, agents)
    ora = oracle.OracleBatch(lv.blob, IMG_N)
    if cells is not None:
        ora.set_placement(cells)
        ora.reset()
    out, flagged = {}, 0
    for k in range(IMG_STEPS):
        ora.step(acts[k], auto_reset=True)
        snap = ora.snapshot_all()
        flagged += int((snap["error"] != 0).sum())
        if k % IMG_EVERY == IMG_EVERY - 1:
            out[k] = {"snapshot": snap}
            for radius in RADII:
                out[k][radius] = ora.obs_image(radius)
    return out, flagged
