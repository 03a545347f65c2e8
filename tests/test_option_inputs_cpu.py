"""No GPU: the conditions the inputs of test_multi_step_options_gpu.py and test_obs_image_gpu.py
(tests/option_inputs.py) must meet, checked with the oracle alone -- so that no GPU case can pass
vacuously -- and the two restatements those tests use as references (the in-kernel partner's PCG32
draw, the episode statistics) against hand-computed values.
"""
import os
import re

import numpy as np
import pytest

import option_inputs as oi
import policy_ref
from conftest import ROOT


# ---- the multi-step inputs ---------------------------------------------------------------------
MULTI = [(lv, cfg) for lv in oi.MULTI_LEVELS for cfg in oi.CONFIGS]


@pytest.mark.parametrize("level,cfg_id", MULTI, ids=["%s-%s" % m for m in MULTI])
def test_multi_step_inputs_reach_what_the_gpu_cases_need(level, cfg_id):
    """Valid actions raise no flag in any env-step; every env finishes at least four episodes; on at
    least 20 of the 60 steps the done row of envs 0..63 -- one wave -- is mixed.  (Measured: 0 flagged,
    4 to 5 episodes per env, 29 mixed steps in every case.  The level placed by the in-kernel generator
    is run on host-drawn cells here; its GPU cases assert the first two conditions on the cells the
    library drew.)"""
    steps = oi.multi_reference(level, cfg_id)
    assert len(steps) == oi.STEPS
    assert sum(int(s["raised"].sum()) for s in steps) == 0
    assert all(int((s["error"] != 0).sum()) == 0 for s in steps)
    done = np.stack([s["done"] for s in steps])
    per_env = done.sum(axis=0)
    assert per_env.min() >= 4, per_env.min()
    wave = done[:, :64].sum(axis=1)
    assert int(((wave > 0) & (wave < 64)).sum()) >= 20
    # (the smaller batches are prefixes: the same holds for envs 0..62, and env 0 alone ends 4 episodes)
    assert per_env[0] >= 4


@pytest.mark.parametrize("cfg_id", ["ego-led", "comm-off"])
def test_invalid_indices_are_flagged_where_the_player_talks(cfg_id):
    """The sprinkled input: both kinds of error-free and flagged env-steps occur, every invalid value
    of the issue's list is present, and an invalid comm index of a silent player alone raises nothing."""
    wide, narrow = oi.multi_actions(True)
    for v in (5, 7, -1, (1 << 32) + 1, -(1 << 40)):
        assert (wide[:, 0] == v).any() and (wide[:, 2] == v).any(), v
    for v in (oi.C, -2, 99, (1 << 32) + 1, -(1 << 40)):
        assert (wide[:, 1] == v).any() and (wide[:, 3] == v).any(), v
    assert narrow.min() >= -2 ** 31 and narrow.max() < 2 ** 31
    steps = oi.multi_reference("open-divider_tomato", cfg_id, True)
    raised = np.stack([s["raised"] for s in steps])
    cfg = oi.config(cfg_id)
    bad_mv = (narrow[:, 0] < 0) | (narrow[:, 0] > 3) | (narrow[:, 2] < 0) | (narrow[:, 2] > 3)
    bad_ego_cm = (narrow[:, 1] < 0) | (narrow[:, 1] >= oi.C)
    bad_alt_cm = (narrow[:, 3] < 0) | (narrow[:, 3] >= oi.C)
    assert raised.sum() > 50 and (raised == 0).sum() > raised.sum()
    silent = bad_alt_cm if cfg["ego_led"] else (bad_ego_cm | bad_alt_cm)      # comm-off: nobody talks
    only_silent = silent & ~bad_mv & ~(bad_ego_cm & bool(cfg["communication_on"]))
    assert only_silent.sum() > 10 and not raised[only_silent].any()
    assert (raised != 0)[bad_mv].sum() > 0 and not (raised != 0)[~bad_mv & ~bad_ego_cm & ~bad_alt_cm].any()


# ---- the image inputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,agents,shape,merges", oi.IMAGE_CASES, ids=oi.IMAGE_IDS)
def test_image_inputs_reach_what_the_gpu_cases_need(name, agents, shape, merges):
    """No env-step is flagged; held, chopped and merged objects occur at compared steps (the 4-agent
    salad and the wide map merge nothing within 120 steps: not required there); at least 50 distinct
    viewer-0 images among the 100 envs at the last compared step."""
    lv = oi.image_level(name, agents)
    assert (lv.width, lv.height) == shape and lv.num_agents == agents
    ref, flagged = oi.image_reference(name, agents)
    assert flagged == 0
    assert sorted(ref) == list(range(oi.IMG_EVERY - 1, oi.IMG_STEPS, oi.IMG_EVERY))
    held = chopped = merged = 0
    for k, rec in ref.items():
        snap = rec["snapshot"]
        held += int((snap["agents"][:, :, 2] >= 0).sum())
        chopped += int((snap["items"][:, :, 2] > 0).sum())
        merged += int((snap["nobj"] < lv.num_items).sum())
    assert held > 0 and chopped > 0, (held, chopped)
    if merges:
        assert merged > 0
    maps, hold = ref[oi.IMG_STEPS - 1][1000]
    assert maps.shape == (2, 7) + shape + (oi.IMG_N,) and hold.shape == (2, oi.IMG_N)
    distinct = {maps[0, ..., i].tobytes() for i in range(oi.IMG_N)}
    assert len(distinct) >= 50, len(distinct)
    # fog: radius 0 shows the viewer's own cell alone, radius 1000 hides nothing
    m0 = ref[oi.IMG_STEPS - 1][0][0]
    assert ((m0[0, 0] != -1).sum(axis=(0, 1)) == 1).all() and (maps != -1).all()


def test_image_oracle_batch_is_the_per_env_function():
    """OracleBatch.obs_image is a loop over oc_oracle_obs_image: env by env the same bytes."""
    from oracle import oracle
    name, agents = "open-divider_tl", 3
    lv = oi.image_level(name, agents)
    acts, _ = oi.image_inputs(name, agents)
    n = 5
    ora = oracle.OracleBatch(lv.blob, n)
    one = [oracle.OracleEnv(lv.blob) for _ in range(n)]
    for k in range(30):
        ora.step(acts[k][:, :n], auto_reset=False)
        for i, e in enumerate(one):
            e.step(acts[k][:, i])
    maps, hold = ora.obs_image(2)
    assert maps.dtype == np.int8 and maps.shape == (2, 7, lv.width, lv.height, n)
    for i, e in enumerate(one):
        for v in range(2):
            m, h = e.obs_image(v, 2)
            assert np.array_equal(maps[v, ..., i], m) and np.array_equal(hold[:, i], h)


# ---- the restatements ----------------------------------------------------------------------------
def _pcg32_scalar(state):
    """PCG32 (RXS-M-XS 32/32) on Python integers."""
    state = (state * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return state, (w >> 22) ^ w


# the first three streams of pcg32_seed_states(7, (130,)) over two steps, worked out by hand with
# _pcg32_scalar: (seed word, [(stream word after the step, move, comm at C = 3)] x 2)
HAND = [(1631897122, [(1609140640, 1, 1), (557950254, 3, 2)]),
        (1626975787, [(3812829025, 1, 2), (2130615015, 3, 0)]),
        (1524890972, [(3640124170, 0, 1), (2166828872, 1, 2)])]


def test_partner_draw_restatement_on_hand_computed_scalars():
    words, mv, cm = oi.partner_stream()
    assert words.shape == (oi.STEPS + 1, oi.NMAX) and mv.shape == cm.shape == (oi.STEPS, oi.NMAX)
    for i, (seed, steps) in enumerate(HAND):
        assert int(words[0, i]) == seed
        s = seed
        for k, (word, move, comm) in enumerate(steps):
            s, o1 = _pcg32_scalar(s)
            s, o2 = _pcg32_scalar(s)
            assert (s, (o1 * 4) >> 32, (o2 * oi.C) >> 32) == (word, move, comm)       # the table itself
            assert int(np.uint32(words[k + 1, i])) == word and int(mv[k, i]) == move and int(cm[k, i]) == comm
    assert mv.min() == 0 and mv.max() == 3 and cm.min() == 0 and cm.max() == oi.C - 1
    # states above 2^31 come back as negative int32 words: the restatement takes them as bit patterns
    s, m, c = oi.partner_draw(np.array([-1, -2 ** 31], np.int32), 5)
    for j, word in enumerate((0xFFFFFFFF, 0x80000000)):
        a, o1 = _pcg32_scalar(word)
        a, o2 = _pcg32_scalar(a)
        assert (int(s[j]), int(m[j]), int(c[j])) == (a, (o1 * 4) >> 32, (o2 * 5) >> 32)


def test_the_steppers_generator_is_the_one_restated():
    """csrc/oc_step_device.h: pcg32 carries the three constants policy_ref.pcg32 restates (that file
    names the policy header's copy).  This reads source text and is only a pointer for whoever changes
    either side; the guard proper is on the GPU, where alt_played and the advanced stream words of
    every step are compared with the restatement (test_multi_step_options_gpu.py, the ego32+rng source)."""
    src = open(os.path.join(ROOT, "gym-comm_amd", "csrc", "oc_step_device.h")).read()
    body = re.search(r"uint32_t\s+pcg32\s*\(\s*uint32_t\s*&\s*state\s*\)\s*\{(.*?)\}", src, re.S).group(1)
    found = {int(c) for c in re.findall(r"\b(\d{6,})u?\b", body)}
    assert found == {policy_ref.PCG_MULT, policy_ref.PCG_INC, policy_ref.PCG_OUT_MULT}
    assert (policy_ref.PCG_MULT, policy_ref.PCG_INC, policy_ref.PCG_OUT_MULT) == (747796405, 2891336453, 277803737)
    s, out = policy_ref.pcg32(np.array([12345], np.int32))
    assert (int(s[0]), int(out[0])) == _pcg32_scalar(12345)


def test_episode_statistics_restatement_on_a_hand_made_stream():
    """ret = where(prev_done, r, ret + r), len = where(prev_done, 1, len + 1): the value stored at a
    step that ends an episode is the finished episode's total; the next step starts over."""
    r = np.array([[0.5, 1.0], [0.25, -2.0], [1.0, 0.125], [3.0, 4.0], [-1.0, 0.5]])
    d = np.array([[0, 0], [1, 0], [0, 0], [0, 1], [1, 0]], np.int32)
    ret, length = oi.stats_reference(r, d)
    assert ret.tolist() == [[0.5, 1.0], [0.75, -1.0], [1.0, -0.875], [4.0, 3.125], [3.0, 0.5]]
    assert length.tolist() == [[1, 1], [2, 2], [1, 3], [2, 4], [3, 1]]
    assert ret.dtype == np.float64 and length.dtype == np.int32
    # left to right in fp64: (0.1 + 0.2) + 0.3, not 0.1 + (0.2 + 0.3)
    ret, _ = oi.stats_reference(np.array([[0.1], [0.2], [0.3]]), np.zeros((3, 1), np.int32))
    assert ret[2, 0] == (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    # one step on given values (the GPU cases that refill the tensors before every step)
    a, b = oi.stats_step([1000.25, 7.0], [41, 9], [0, 1], [0.5, 0.5])
    assert a.tolist() == [1000.75, 0.5] and b.tolist() == [42, 1]
