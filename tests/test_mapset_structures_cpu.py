"""No GPU: map sets on the structures test_mapset_structures_gpu.py steps (tests/mapset_inputs.py).

  from_maps, with the constructor stubbed, accepts the sets the GPU cases build -- the eight shipped
    random-*_salad levels, the two random-*_tomato levels, three Salad maps compiled with a time limit
    each, custom-two_tomatoes beside a variant written in mapset_inputs.py -- and refuses, naming both
    levels, pairs whose structure differs;
  the nominal placement of placement_mode="host" is per env: each env its OWN map's first Counters;
  with the oracle alone, every case's inputs reach what the GPU case is about, so that none can pass
    vacuously (the in-kernel draw is stood in for by a host pattern here)."""
import numpy as np
import pytest

import mapset_inputs as mi
from test_mapset_cpu import no_batch  # noqa: F401  (the fixture)


# ---- from_maps ---------------------------------------------------------------------------------
def test_the_shipped_random_families_and_the_new_sets_are_accepted(no_batch):  # noqa: F811
    B, seen = no_batch
    B.from_maps(mi.SALAD8, num_envs=8 * 64)
    B.from_maps(mi.RANDOM_TOMATO, num_envs=100)
    B.from_maps(mi.case_levels("per-map-T"), num_envs=229, group_map=[0, 1, 2, 1])
    B.from_maps(mi.case_levels("dup"), num_envs=229, group_map=[0, 1, 1, 0])
    B.from_maps(mi.TL, num_envs=229, subtask_order=mi.TL_ORDER)
    salad, tomato, per_t, dup, tl = seen
    assert [m.name for m in salad[1]["_maps"][0]] == mi.SALAD8 and salad[1]["_maps"][1].tolist() == list(range(8))
    assert sorted(len(m.counters) for m in salad[1]["_maps"][0]) == [9, 14, 17, 19, 20, 20, 23, 29]
    assert [(m.width, m.height) for m in salad[1]["_maps"][0]] == [(5, 5), (6, 5), (7, 7), (11, 4), (7, 7), (7, 7),
                                                                   (9, 5), (8, 7)]
    assert [m.name for m in tomato[1]["_maps"][0]] == mi.RANDOM_TOMATO
    assert [m.max_num_timesteps for m in per_t[1]["_maps"][0]] == [12, 25, 40]
    assert all(m.has_dup for m in dup[1]["_maps"][0]) and dup[0].name == "custom-two_tomatoes"
    assert [m.num_subtasks for m in tl[1]["_maps"][0]] == [6, 6, 6]


def test_the_dup_variant_is_another_map_of_the_same_structure():
    from gym_comm_amd import _lib, specialize
    a, b = mi.case_levels("dup")
    assert specialize.spec_header_text(a.blob, geometry=False) == specialize.spec_header_text(b.blob, geometry=False)
    assert _lib.subtask_info(a.blob) == _lib.subtask_info(b.blob) and _lib.subtask_info(a.blob)[2]       # dup
    assert (a.width, a.height) == (b.width, b.height) == (7, 7)
    assert [t for t, _, _ in a.items] == [t for t, _, _ in b.items]
    assert a.delivery != b.delivery and not np.array_equal(a.cells, b.cells)
    assert [(x, y) for _, x, y in a.items] != [(x, y) for _, x, y in b.items]
    assert specialize.spec_header_text(a.blob, geometry=True) != specialize.spec_header_text(b.blob, geometry=True)


@pytest.mark.parametrize("pair", [("random-open-divider_salad", "random-open-divider_tomato"),
                                  ("custom-two_tomatoes", "custom-two_tomatoes_small")])
def test_pairs_of_different_structure_are_refused_by_name(no_batch, pair):  # noqa: F811
    B, seen = no_batch
    lvs = [mi.compiled(m, 25) for m in pair]
    with pytest.raises(ValueError) as e:
        B.from_maps(lvs, num_envs=128)
    assert all(lv.name in str(e.value) for lv in lvs) and lvs[0].name != lvs[1].name
    assert not seen


# ---- the nominal placement ---------------------------------------------------------------------
def test_nominal_placement_is_each_envs_own_maps():
    """placement_mode="host" starts every env on the cells its map was compiled with -- the first
    Counters of THAT map.  (Built from the first map alone, env 70 of this set would start on (2, 0) of
    the 5 x 5 map: a Cutboard.)"""
    from gym_comm_amd.batched import nominal_placement
    names = [mi.SALAD8[2], mi.SALAD8[0], mi.SALAD8[3], mi.SALAD8[7]]         # 7 x 7, 5 x 5, 11 x 4, 8 x 7
    lvs = [mi.compiled(m, 25) for m in names]
    gm, n = [0, 1, 2, 3], 229
    got = nominal_placement(lvs, gm, n)
    assert got.dtype == np.int32 and got.shape == (3, n) and got.flags["C_CONTIGUOUS"]
    for i in range(n):
        lv = lvs[gm[i // 64]]
        assert got[:, i].tolist() == lv.pack_placement([(x, y) for _, x, y in lv.items]), i
        assert set(got[:, i].tolist()) <= set(mi.counter_cells(lv).tolist())
    assert sorted(got[:, 3].tolist()) == [1, 2, 3] and sorted(got[:, 70].tolist()) == [1, 3, 16]
    assert (got[:, 3] != got[:, 70]).any()
    assert lvs[1].cells[0][2] != lvs[1].cells[0][1]         # (2, 0) of the small map is no Counter
    # one level: every env the level's own column
    assert np.array_equal(nominal_placement(lvs[1:2], None, 5), np.repeat(got[:, 70:71], 5, axis=1))


# ---- what the GPU cases' inputs reach ------------------------------------------------------------
def _totals(case):
    names, Ts, gm, n, steps, _ = mi.CASES[case]
    ref = mi.reference(case)[1:]
    em = mi.env_map(case)
    done = np.stack([r["done"] for r in ref])
    raised = np.stack([r["raised"] for r in ref])
    completed = np.zeros(len(names), np.int64)
    for r in ref:
        for m, counts in r["per_map"]:
            completed[m] += counts["completed_subtasks_sum"]
    return names, Ts, em, steps, done, raised, completed, ref


@pytest.mark.parametrize("case", sorted(mi.CASES))
def test_inputs_reach_what_the_gpu_cases_need(case):
    """No env-step is flagged except on the cramped map; every env finishes at least steps // T episodes
    of its own map's T; some subtask is completed on every map.  (Seed 23: 15 to 104 completed subtasks
    per Salad map over 229 x 120 env-steps, no success: none is required.)"""
    names, Ts, em, steps, done, raised, completed, ref = _totals(case)
    for m, name in enumerate(names):
        on = em == m
        assert on.any(), name
        if name == mi.CRAMPED:
            assert raised[:, on].sum() > 100
            assert any((r["snapshot"]["error"][on] != 0).any() for r in ref)
        else:
            assert raised[:, on].sum() == 0, name
            assert all((r["snapshot"]["error"][on] == 0).all() for r in ref), name
        assert done[:, on].sum(axis=0).min() >= steps // Ts[m], name
        assert completed[m] > 0, name


def test_per_map_time_limits_leave_the_batch_out_of_lockstep():
    """Maps with T = 12, 25 and 40, two thirds of the T = 25 map's envs 5 and 9 steps behind after a reset by hand:
    an env times out at its OWN map's T, the done row is mixed (some envs done, some not) on at least 20
    of the 120 steps, and the timestep row is t / T of that T."""
    names, Ts, em, steps, done, raised, completed, ref = _totals("per-map-T")
    mixed = int(((done.sum(axis=1) > 0) & (done.sum(axis=1) < done.shape[1])).sum())
    assert mixed >= 20, mixed
    n = len(em)
    t_env = np.asarray(Ts)[em]
    behind = np.zeros(n, np.int64)          # how many steps an env lags its map after its reset by hand
    for k in mi.STAGGER:
        behind[mi.stagger_mask("per-map-T", k) != 0] = k + 1
    assert sorted(set(behind.tolist())) == [0, 5, 9] and set(em[behind > 0].tolist()) == {1}
    assert all(np.count_nonzero(behind[64 * g:64 * g + 64] == b) for g in (1, 3) for b in (0, 5, 9))
    delivered = np.stack([r["success"] for r in ref]).any(axis=0)
    assert (~delivered).sum() > n // 2
    for k in range(steps):
        t = k + 1 - np.where(k + 1 > behind, behind, 0)         # steps since the env's last reset by hand
        timeout = t % t_env == 0
        assert np.array_equal(done[k][~delivered] != 0, timeout[~delivered]), k
        live = ~delivered & ~timeout
        assert (ref[k]["timestep"][live] == (t % t_env)[live] / t_env[live].astype(np.float64)).all(), k
    # the three limits really are told apart by the rows: after step 0 three different timestep values
    assert len(set(ref[0]["timestep"].tolist())) == 3


def test_the_dup_scripts_reach_goal_counts_of_two_and_merged_objects():
    names, Ts, em, steps, done, raised, completed, ref = _totals("dup")
    lvs = mi.case_levels("dup")
    for m, lv in enumerate(lvs):
        on = em == m
        two = sum(int((r["snapshot"]["goal_count"][on] >= 2).any(axis=1).sum()) for r in ref)
        merged = sum(int((r["snapshot"]["nobj"][on] < lv.num_items).sum()) for r in ref)
        assert two > 0 and merged > 0, (lv.name, two, merged)
    assert raised.sum() == 0


def test_the_host_pattern_uses_every_counter_and_distinct_cells():
    for case in ("family", "host", "vec-env"):
        lvs, em = mi.case_levels(case), mi.env_map(case)
        first = mi.host_cells(case, -1)
        for cells in (first, mi.host_cells(case, 0), mi.host_cells(case, 7)):
            assert cells.dtype == np.int32 and cells.shape == (3, len(em))
            assert all(len(set(cells[:, i].tolist())) == 3 for i in range(len(em)))
            for m, lv in enumerate(lvs):
                assert np.isin(cells[:, em == m], mi.counter_cells(lv)).all()
        for m, lv in enumerate(lvs):        # 3 i + k mod c over at least 37 envs: every Counter of every map
            assert set(first[:, em == m].reshape(-1).tolist()) == set(mi.counter_cells(lv).tolist()), lv.name
        assert not np.array_equal(mi.host_cells(case, 0), mi.host_cells(case, 7))


def test_tl_rows_in_the_callers_order_are_the_canonical_rows_permuted():
    """The reference of the tl case, compiled in the caller's subtask order, against a second run in the
    canonical order: row j of completed_subtasks is the canonical row TL_ORDER[j]; everything else is equal."""
    from test_mapset_gpu import SetOracle
    names, Ts, gm, n, steps, _ = mi.CASES["tl"]
    acts, _ = mi.actions("tl")
    ref = mi.reference("tl")[1:]
    ora = SetOracle([mi.compiled(m, T) for m, T in zip(names, Ts)], gm, n)
    ora.reset()
    lo, S = 16, 6           # batched.obs_layout: four 4-row keys in front of completed_subtasks
    seen = 0
    for k in range(steps):
        r = ora.multi_step(acts[k])
        want = r["obs"].copy()
        want[:, lo:lo + S] = r["obs"][:, lo:lo + S][:, mi.TL_ORDER]
        assert np.array_equal(ref[k]["obs"], want), k
        assert np.array_equal(ref[k]["reward"].view(np.uint64), r["reward"].view(np.uint64)), k
        assert np.array_equal(ref[k]["snapshot"]["completed"], r["snapshot"]["completed"][:, mi.TL_ORDER]), k
        seen += int(r["obs"][:, lo:lo + S].sum())
    assert seen > 0 and mi.TL_ORDER != sorted(mi.TL_ORDER)
