"""-m gpu: the fused step's GENERAL variant (csrc/oc_kernels.hip: select_multi, XO = 2) with its
options in use, against ``oracle.OracleBatch.multi_step`` bit for bit, every step.

``OvercookedVecEnv`` never launches the plain step: it passes [n][2] action pairs, keeps episode
statistics and often draws the partner in the kernel, and any non-standard wrapper configuration
(ego-led, communication off, ego_agent_idx = 1, a BLIND or non-moving player, play) selects the
general variant.  The rest of the suite exercises the two halves apart -- non-standard
configurations with the four action rows, options on the standard configuration -- so this file
crosses them (tests/option_inputs.py holds the inputs; tests/test_option_inputs_cpu.py checks on the
CPU that they end episodes, desynchronise the batch and raise no flag):

  six wrapper configurations that together flip every axis, C = 3, radius 1;
  five action sources carrying the SAME actions: the four rows; int32 pairs; int64 pairs; ego int32
    pairs + partner rows (the ego's rows then hold other moves, which must be ignored); ego int32
    pairs + the in-kernel partner.  The partner's actions are the draw itself, restated in numpy
    (option_inputs.partner_draw), so one oracle run serves every source, and alt_played and the
    advanced stream words are asserted against that restatement;
  episode statistics on (one control per library without), against numpy fp64;
  the generic library (one wave), specialised libraries with launch hints 4 and 1, one case with
    hint 2 (no such kernel: one wave); the three observation dtypes rotate over the cases;
  two fixed levels and one placed by the in-kernel generator (the cells are read back from the
    state and handed to the oracle);
  T = 12 and 60 steps -- four or five episodes per env -- and, after each of the first six steps, a
    masked reset of every seventh env, so that the envs of a wave end their episodes on different steps;
  n = 130 (two workgroups, a two-env tail) for the full product; n = 63 and n = 1 (an 8-byte pair
    buffer under the 16-byte load) with alt_played and the statistics refilled before every step and,
    like the stream words, placed in front of guard bytes;
  about 1 % invalid indices, int64 values outside int32 among them: the same error bits on the same
    envs as the oracle.

Variants reached, as (library, XO, waves per 64 envs): (generic, 2, 1), (specialised, 2, 4),
(specialised, 2, 1), each with every source and every observation dtype.
"""
import numpy as np
import pytest
import torch

import option_inputs as oi
from hip_util import SENTINEL, assert_snapshots_equal, bits
from hip_util import with_margin as _with_margin

pytestmark = pytest.mark.gpu

C, STEPS, RADIUS = oi.C, oi.STEPS, oi.RADIUS
FILL = 0x6B
DTYPES = [torch.int32, torch.int8, torch.float32]
CFG_IDS = list(oi.CONFIGS)
SOURCES = ["rows", "pairs32", "pairs64", "ego32+rows", "ego32+rng"]
# library id -> (specialize_level, launch hint, flavour, waves per 64 envs of the general variant)
LIBS = {"generic": (False, 0, "generic", 1), "spec4": (True, 4, "spec", 4), "spec1": (True, 1, "spec", 1),
        "spec2": (True, 2, "spec", 1)}
COUNTERS = ("env_steps", "episodes", "successes", "reward_sum", "completed_subtasks_sum", "errors")


def _dtype(cfg_id, source, lib):
    """int32 / int8 / float32 in rotation: with a library fixed, every dtype meets every source."""
    return DTYPES[(CFG_IDS.index(cfg_id) + SOURCES.index(source) + list(LIBS).index(lib)) % 3]


def _state_cells(env):
    """Packed item cells (x | y<<4) [M][n] read back from the device state."""
    w = env.state[env.A:env.A + env.M].cpu().numpy()
    return np.ascontiguousarray((w & 255).astype(np.int32))


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to("cuda:0")      # (a copy: the inputs are read-only)


def _run(monkeypatch, level, lib, cfg_id, source, n, stats=True, guard=False, invalid=False):
    from gym_comm_amd.batched import BatchedOvercooked
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    cfg = oi.config(cfg_id)
    spec, hint, flavour, waves = LIBS[lib]
    lv = oi.multi_level(level, cfg["play"])
    dtype = _dtype(cfg_id, source, lib)
    env = BatchedOvercooked(lv, num_envs=n, device="cuda:0", num_communication=C, fow_radius=RADIUS,
                            communication_on=cfg["communication_on"], ego_led=cfg["ego_led"],
                            ego_agent_idx=cfg["ego_agent_idx"], ego_config=cfg["ego"],
                            partner_config=cfg["partner"], auto_reset=True, obs_dtype=dtype,
                            episode_stats=stats, specialize_level=spec, waves_per_64=hint,
                            placement_mode="rng", seed=11)
    assert env.kernel_flavour == flavour
    assert not env.standard_wrapper_config
    assert env.launch_waves(general=True) == waves and env.launch_lanes(general=True) == 1
    case = "%s %s %s %s n=%d %s" % (level, lib, cfg_id, source, n, str(dtype)[6:])
    if invalid:
        wide, narrow = oi.multi_actions(True)
    else:
        wide = narrow = oi.multi_actions()
    wide, narrow = wide[:, :, :n], narrow[:, :, :n]
    live = None
    if lv.random_placement:
        counters = {x | (y << 4) for x, y in lv.counters}
        cells = _state_cells(env)
        assert set(np.unique(cells).tolist()) <= counters
        live = oi.MultiReference(level, cfg_id, n, cells=cells)
        assert_snapshots_equal(env.snapshot(), live.ora.snapshot_all(), case + " after reset")
    else:
        ref_steps = oi.multi_reference(level, cfg_id, invalid)
    words, p_mv, p_cm = oi.partner_stream()
    margins = {}
    stream = played = None
    if source == "ego32+rng":
        stream, margins["alt_rng"] = _with_margin(_dev(words[0, :n], torch.int32))
        played, margins["alt_played"] = _with_margin(torch.zeros((2, n), dtype=torch.int32, device="cuda:0"))
    if guard and stats:      # (before the first step: it fixes the pointers it launches with)
        env.ep_return, margins["ep_return"] = _with_margin(env.ep_return)
        env.ep_length, margins["ep_length"] = _with_margin(env.ep_length)
    ret_pat = 1000.25 + 0.5 * np.arange(n)
    len_pat = (100000 + np.arange(n)).astype(np.int32)
    ret, length, prev_done = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    totals = dict.fromkeys(COUNTERS, 0)
    episodes = np.zeros(n, np.int64)          # per env
    for k in range(STEPS):
        ctx = "%s step %d" % (case, k)
        if guard:
            if played is not None:
                played.view(torch.uint8).fill_(FILL)
            if stats:
                env.ep_return.copy_(_dev(ret_pat, torch.float64))
                env.ep_length.copy_(_dev(len_pat, torch.int32))
                ret, length = ret_pat, len_pat
        a = wide[k]
        if source == "rows":
            out = env.multi_step(_dev(narrow[k], torch.int32))
        elif source in ("pairs32", "pairs64"):
            dt, src = (torch.int32, narrow[k]) if source == "pairs32" else (torch.int64, a)
            out = env.multi_step(None, ego_pairs=_dev(src[0:2].T, dt), alt_pairs=_dev(src[2:4].T, dt))
        elif source == "ego32+rows":
            rows = narrow[k].copy()
            rows[0], rows[1] = 3 - rows[0], (rows[1] + 1) % C      # where the ego is NOT read from
            out = env.multi_step(_dev(rows, torch.int32), ego_pairs=_dev(narrow[k][0:2].T, torch.int32))
        else:
            out = env.multi_step(None, ego_pairs=_dev(narrow[k][0:2].T, torch.int32), alt_rng=stream,
                                 alt_played=played)
        o, t, r, d = out
        if live is not None:
            ref = live.step(k, _state_cells(env))
        else:
            ref = {key: (v[..., :n] if isinstance(v, np.ndarray) else v) for key, v in ref_steps[k].items()}
        got = o.cpu().numpy()
        assert got.shape == ref["obs"].shape and o.dtype == dtype, ctx
        assert np.array_equal(d.cpu().numpy(), ref["done"]), ctx
        assert np.array_equal(got.astype(np.int64), ref["obs"].astype(np.int64)), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(ref["timestep"])), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ref["reward"])), ctx
        assert np.array_equal(env.comm.cpu().numpy(), ref["comm"]), ctx
        assert np.array_equal(env.reward.cpu().numpy(), ref["sparse"]), ctx
        hs = None
        if invalid or lv.random_placement or k % oi.SNAP_EVERY == oi.SNAP_EVERY - 1 or k == STEPS - 1:
            hs = env.snapshot()
            snap = ref["snapshot"] if live is not None else {key: v[:n] for key, v in ref["snapshot"].items()}
            assert np.array_equal(hs["error"], snap["error"]), ctx      # the same bits on the same envs
            assert_snapshots_equal(hs, snap, ctx)
        if not invalid:
            assert int(ref["raised"].sum()) == 0 and int((ref["error"] != 0).sum()) == 0, ctx
        if stats:
            ret, length = oi.stats_step(ret, length, prev_done, ref["reward"])
            assert np.array_equal(bits(env.ep_return.cpu().numpy()), bits(ret)), ctx
            assert np.array_equal(env.ep_length.cpu().numpy(), length), ctx
        else:
            assert env.ep_return is None and env.ep_length is None
        prev_done = ref["done"]
        if stream is not None:
            assert np.array_equal(stream.cpu().numpy(), words[k + 1, :n]), ctx
            assert np.array_equal(played.cpu().numpy(), np.stack([p_mv[k, :n], p_cm[k, :n]])), ctx
        totals["env_steps"] += n
        totals["episodes"] += int(ref["done"].sum())
        episodes += ref["done"] != 0
        totals["successes"] += int(ref["success"].sum())
        totals["reward_sum"] += int(ref["sparse"].sum())
        totals["completed_subtasks_sum"] += int(ref["completed"].sum())
        totals["errors"] += int(ref["raised"].sum())
        mask = oi.stagger_mask(k, n)
        if mask is not None and mask.any():
            env.reset(_dev(mask, torch.int32))
            if live is not None:
                live.reset(mask, _state_cells(env))
                assert_snapshots_equal(env.snapshot(), live.ora.snapshot_all(), ctx + " after the masked reset")
    for name, m in margins.items():
        assert bool((m == SENTINEL).all().item()), "%s: bytes past the end of %s were written" % (case, name)
    m = env.read_metrics()
    assert {c: m[c] for c in COUNTERS} == totals, case
    assert episodes.min() >= 4, case           # EVERY env ended four episodes (on the cells the library drew, too)
    return totals


FIXED = oi.MULTI_LEVELS[:2]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cfg_id", CFG_IDS)
@pytest.mark.parametrize("lib", ["generic", "spec4", "spec1"])
@pytest.mark.parametrize("level", FIXED)
def test_general_variant_with_options_matches_oracle(monkeypatch, level, lib, cfg_id, source):
    _run(monkeypatch, level, lib, cfg_id, source, oi.NMAX)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("cfg_id", CFG_IDS)
@pytest.mark.parametrize("lib", ["generic", "spec4"])
def test_general_variant_on_a_level_placed_by_the_kernel(monkeypatch, lib, cfg_id, source):
    """placement_mode="rng": the split launch's placement draw (every wave draws the same cells from
    its copy of the stream word) in the general variant; masked oc_reset re-places per env."""
    _run(monkeypatch, oi.RNG_LEVEL, lib, cfg_id, source, oi.NMAX)


SMALL = [(n, lib, source, CFG_IDS[(si + li + (n == 1)) % len(CFG_IDS)], FIXED[(si + li) % 2])
         for n in (1, 63) for li, lib in enumerate(["generic", "spec4", "spec1"]) for si, source in enumerate(SOURCES)]


@pytest.mark.parametrize("n,lib,source,cfg_id,level", SMALL,
                         ids=["n%d-%s-%s-%s" % s[:4] for s in SMALL])
def test_small_batches_write_nothing_but_their_own_words(monkeypatch, n, lib, source, cfg_id, level):
    """One lone env (its int32 pair is 8 bytes under a 16-byte load) and a wave one env short:
    alt_played and the statistics hold a pattern before every step -- a word nobody stored shows, and
    the statistics' one-step function is checked on values the kernel has never produced -- and they
    and the stream words end in front of guard bytes."""
    _run(monkeypatch, level, lib, cfg_id, source, n, guard=True)


@pytest.mark.parametrize("lib", ["generic", "spec4", "spec1"])
def test_control_without_episode_statistics(monkeypatch, lib):
    _run(monkeypatch, "open-divider_tomato", lib, "ego-led", "pairs32", oi.NMAX, stats=False)


def test_hint_two_falls_back_to_one_wave(monkeypatch):
    """No library holds a two-way split of the general variant: the hint launches one wave."""
    _run(monkeypatch, "full-divider_salad", "spec2", "all-flipped", "ego32+rng", oi.NMAX)


@pytest.mark.parametrize("lib,cfg_id,source", [("spec4", "ego-led", "pairs64"), ("generic", "comm-off", "pairs64"),
                                               ("spec1", "ego-led", "rows")])
def test_invalid_indices_raise_the_oracles_flags(monkeypatch, lib, cfg_id, source):
    """About 1 % invalid move and comm indices in every row -- as int64 pairs also values whose low
    word alone would be valid: the same error bits on the same envs every step, the defined result
    (nothing sent, no move), and the errors counter.  A bad comm index of a player who does not talk
    (the partner when ego-led, both with communication off) raises nothing."""
    totals = _run(monkeypatch, "open-divider_tomato", lib, cfg_id, source, oi.NMAX, invalid=True)
    assert totals["errors"] > 50
