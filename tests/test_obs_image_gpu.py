"""-m gpu: the image observation kernel (csrc/oc_step_device.h: k_obs_image) against the oracle's
``oc_oracle_obs_image`` (``OracleBatch.obs_image``), byte for byte, on batches whose envs all differ.

The kernel works quad by quad -- four consecutive cells of a plane per dword -- and was so far
checked by two 2-agent golden tapes with every env in the same state.  What its per-lane parts can
get wrong: the quad an agent or item falls into and its byte there; the fog bytes at the radius'
edge; agent planes 3 and 4 overwriting the content planes with three or four agents; an item giving
way to a LATER item of its type on the same cell (levels that repeat a type); the x-major cell
index on maps with W != H; the last quad where W*H is no multiple of four.  So: seven levels
(tests/option_inputs.py: IMAGE_CASES -- 2, 3 and 4 agents, 7x7, 11x4, 8x7 and 5x5 maps, two levels
that repeat a type), 100 envs (a 36-lane tail) with per-env action streams and auto-reset, per-env
placements on the random-* levels; every 10 of 120 steps the images and holding flags of all envs at
radii 0, 1, 2, 5 and 1000, on the generic and the specialised library.  tests/
test_option_inputs_cpu.py checks that held, chopped and merged objects occur and that the envs differ.

"Specialised" is whatever ``specialize.load_for`` finds for the level, and nothing is compiled at test
time: the LEVEL library (map folded in) for the six levels tests/spec_levels.py lists -- T is a
run-time argument and selects nothing --, the STRUCTURE library that build() makes for every built-in
level (map a run-time argument) for random-open-divider_salad_small_wide_big, which that file does
not list.  Both instantiate k_obs_image<A, M, DUP> for the one (A, M, DUP) of the level; the cases
assert the flavour, not which of the two was reached.
"""
import numpy as np
import pytest
import torch

import option_inputs as oi
from hip_util import assert_snapshots_equal

pytestmark = pytest.mark.gpu


def _run(name, agents, spec, check):
    """Step the library through the case's actions beside nothing: the oracle's side is cached
    (option_inputs.image_reference).  `check(env, step, reference record)` at every compared step."""
    from gym_comm_amd.batched import BatchedOvercooked
    lv = oi.image_level(name, agents)
    acts, cells = oi.image_inputs(name, agents)
    ref, flagged = oi.image_reference(name, agents)
    assert flagged == 0
    env = BatchedOvercooked(lv, num_envs=oi.IMG_N, device="cuda:0", auto_reset=True, specialize_level=spec,
                            placement_mode="host")
    assert env.kernel_flavour == ("spec" if spec else "generic")
    if cells is not None:
        env.set_placement(torch.from_numpy(cells.copy()).to("cuda:0"))
        env.reset()
    acts_d = torch.from_numpy(acts.copy()).to("cuda:0")
    for k in range(oi.IMG_STEPS):
        env.step(acts_d[k])
        if k in ref:
            assert_snapshots_equal(env.snapshot(), ref[k]["snapshot"], "%s step %d" % (name, k))
            check(env, k, ref[k])
    return env


@pytest.mark.parametrize("spec", [False, True], ids=["generic", "spec"])
@pytest.mark.parametrize("name,agents,shape,merges", oi.IMAGE_CASES, ids=oi.IMAGE_IDS)
def test_images_match_oracle_env_by_env(name, agents, shape, merges, spec):
    seen = {"fogged": 0}

    def check(env, k, rec):
        for radius in oi.RADII:
            maps, hold = env.observe_image(radius)
            m, h = maps.cpu().numpy(), hold.cpu().numpy()
            mo, ho = rec[radius]
            ctx = "%s step %d radius %d" % (name, k, radius)
            assert m.dtype == np.int8 and m.shape == mo.shape == (2, 7) + shape + (oi.IMG_N,), ctx
            if not np.array_equal(m, mo):
                v, p, x, y, i = (int(c) for c in np.argwhere(m != mo)[0])
                raise AssertionError("%s: viewer %d plane %d cell (%d, %d) env %d: %d, oracle %d"
                                     % (ctx, v, p, x, y, i, m[v, p, x, y, i], mo[v, p, x, y, i]))
            assert np.array_equal(h.astype(np.int32), ho), ctx
            seen["fogged"] += int((mo == -1).sum())

    _run(name, agents, spec, check)
    assert seen["fogged"] > 0


@pytest.mark.parametrize("name,agents", [("open-divider_tl", 3), ("random-open-divider_salad_small", 2)],
                         ids=["7x7", "5x5"])
def test_packed_form_pads_the_last_quad_with_zeros(name, agents):
    """packed=True returns the kernel's own tensor, int32 [2][7 * ceil(W*H / 4)][n]: byte b of word q of
    a plane is cell 4 q + b; W*H = 49 and 25 leave three padding bytes in the last quad, which are
    zero whatever the fog says, and the cells in front of them are the oracle's."""
    lv = oi.image_level(name, agents)
    cells = lv.width * lv.height
    q = (cells + 3) // 4
    assert cells % 4 == 1

    def check(env, k, rec):
        for radius in (0, 2, 1000):
            packed, _ = env.observe_image(radius, packed=True)
            assert packed.dtype == torch.int32 and tuple(packed.shape) == (2, 7 * q, oi.IMG_N)
            b = packed.cpu().numpy().view(np.uint8).reshape(2, 7, q, oi.IMG_N, 4)    # little-endian bytes
            flat = np.moveaxis(b, 4, 3).reshape(2, 7, 4 * q, oi.IMG_N).view(np.int8)
            ctx = "%s step %d radius %d" % (name, k, radius)
            assert (flat[:, :, cells:] == 0).all(), ctx
            mo = rec[radius][0].reshape(2, 7, cells, oi.IMG_N)
            assert np.array_equal(flat[:, :, :cells], mo), ctx

    _run(name, agents, True, check)


@pytest.mark.parametrize("spec", [False, True], ids=["generic", "spec"])
def test_later_item_of_a_type_wins_on_a_shared_cell_staged(spec):
    """The `later` rule: every object writes its contents' planes in world order (overcooked_env.py:
    171-178), so of two items of one type on one cell the LATER object's value stays.  Merged foods
    are all chopped and a tile holds one object, so the two values differ only where two agents
    stand on one cell (three agents pass through each other's cells; the alias corner of
    test_hip_parity.py) holding a fresh and a chopped food of the same type -- which random play
    practically never reaches.  Staged on the three-tomato level: agent 1 on agent 0's cell (agent 2
    would write its own plane, 3, over the tomatoes'), every ordered pair of tomatoes in their hands,
    either one chopped; one env per combination."""
    from gym_comm_amd.batched import BatchedOvercooked
    from oracle import oracle
    name, agents = "cbase_dup_three_tomatoes_a3", 3
    lv = oi.image_level(name, agents)
    A, M = lv.num_agents, lv.num_items
    toms = [i for i, (t, _, _) in enumerate(lv.items) if t == 0]
    assert len(toms) == 3 and lv.has_dup
    combos = [(i, j, c) for i in toms for j in toms if i != j for c in (0, 1)]
    n = len(combos)
    env = BatchedOvercooked(lv, num_envs=n, device="cuda:0", auto_reset=False, specialize_level=spec)
    assert env.kernel_flavour == ("spec" if spec else "generic")
    ora = oracle.OracleBatch(lv.blob, n)
    start = ora.snapshot_all()
    w = env.state.cpu().numpy().copy()                 # packed words (include/oc_hip.h)
    for e, (i, j, c) in enumerate(combos):
        ag = [[int(v) for v in start["agents"][e, a]] for a in range(A)]
        ag[1][0], ag[1][1] = ag[0][0], ag[0][1]
        ag[0][2], ag[1][2] = i, j
        items = [[int(start["items"][e, m, 0]), int(start["items"][e, m, 1]), 0] for m in range(M)]
        items[i][2], items[j][2] = c, 1 - c
        one = oracle.OracleEnv.__new__(oracle.OracleEnv)
        one.A, one.M, one.S, one._h = ora.A, ora.M, ora.S, ora._handles[e]
        try:
            one.debug_set(ag, items)
        finally:
            one._h = None
        for a, (x, y, h) in enumerate(ag):
            w[a, e] = (w[a, e] & ~0xFFF) | x | (y << 4) | ((h + 1) << 8 if h >= 0 else 0)
        for m, (x, y, st) in enumerate(items):
            holder = [a for a in range(A) if ag[a][2] == m]
            if holder:
                x, y = ag[holder[0]][0], ag[holder[0]][1]
            w[A + m, e] = (w[A + m, e] & ~(0xFF | 0x100 | 0x7000)) | x | (y << 4) | (st << 8) | \
                          (((holder[0] + 1) if holder else 0) << 12)
    env.state.copy_(torch.from_numpy(w).to("cuda:0"))
    assert_snapshots_equal(env.snapshot(), ora.snapshot_all(), "staged state")
    differ = 0
    for radius in (0, 1, 1000):
        maps, hold = env.observe_image(radius)
        mo, ho = ora.obs_image(radius)
        assert np.array_equal(maps.cpu().numpy(), mo), radius
        assert np.array_equal(hold.cpu().numpy().astype(np.int32), ho), radius
    mo, _ = ora.obs_image(1000)
    for e, (i, j, c) in enumerate(combos):     # the cell shows ONE of the two values, and both occur as the winner
        x, y = (int(v) for v in start["agents"][e, 0, :2])
        assert mo[1, 3, x, y, e] in (1, 2)
        differ += int(mo[1, 3, x, y, e] == 1)
    assert 0 < differ < n
