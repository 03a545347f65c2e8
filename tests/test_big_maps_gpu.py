"""-m gpu: maps above 64 cells (tests/big_maps.py) against the CPU oracle, on bits.

Above 64 cells the tile bit-planes take both 64-bit words (`planes128`: cell_type(), env_step's
navigation; in a specialised build a compile-time choice, so instantiations of their own), coordinates
reach 15, W = 16 makes dense()'s multiplier 0, the distance table grows to 16 KB (row offsets up to
127 * 128 + 127), MAX_PATH to 49 and 1 / MAX_PATH with it, the table image to 16 960 bytes -- the
strided tail of the LDS copy -- and the image kernel writes 32 words per plane.  The golden replays
(test_hip_parity.py) step every env of a batch with the same actions; here every env differs:

  seeded runs, n = 229 (a 37-env last group), T = 30, 120 steps (every env auto-resets four times), every
    third env walking its agent 0 to the far column / row first (asserted on the oracle's snapshots):
    the base step with 2, 3 and 4 agents and the fused step with both viewers' rows, on the generic, the
    level and the structure library, on one, two and four waves per 64 envs and the lane-split launch,
    int8 and float32 rows once each;
  the same runs with the tables staged in LDS by 64- and by 256-thread workgroups (128-cell maps: the
    copy's strided loop runs 13 times per thread at 64 threads and once for 36 threads at 256, where
    it moves exactly the probe table and the Counter bytes -- so also on the level that repeats a type
    and on the one that scatters its items);
  fog radius 0, 3 and 1000 on the 16 x 8 map with the partner BLIND;
  oc_obs_image on 16 x 8, 8 x 16 and 11 x 11 at radius 3, with a guard margin behind the output;
  items scattered over 49 Counters: host-supplied placements that use every Counter, and the in-kernel
    draw read back and handed to the oracle, every Counter drawn;
  a map set of two maps above 64 cells; a 64-cell control on the generic library."""
import numpy as np
import pytest
import torch

import big_maps as bm
from hip_util import SENTINEL, assert_snapshots_equal, bits, with_margin

pytestmark = pytest.mark.gpu

N, STEPS = bm.N, bm.STEPS
LIBS = {"generic": False, "level": True, "structure": "structure"}
FLAVOUR = {"generic": 0, "structure": 1, "level": 2}           # oc_is_specialized()
DTYPES = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _env(lv, lib, **kw):
    from gym_comm_amd import specialize
    from gym_comm_amd.batched import BatchedOvercooked
    if lib != "generic":        # build() made it: nothing is compiled at test time
        assert specialize.ensure(lv.blob, geometry=(lib == "level"), compile=False), "%s library of %s" % (lib, lv.name)
    env = BatchedOvercooked(lv, num_envs=kw.pop("n", N), device="cuda:0", auto_reset=True, specialize_level=LIBS[lib], **kw)
    assert env._L.oc_is_specialized() == FLAVOUR[lib]
    return env


def _run_base(name, agents, lib, policy, monkeypatch, placement=None):
    monkeypatch.setenv("OC_LAUNCH", policy)
    lv = bm.level(name, agents)
    assert lv.width * lv.height > 64 or name == "control_8x8"
    ref = bm.base_reference(name, agents, None if placement is None else placement.tobytes())
    kw = {} if placement is None else {"placement_mode": "host"}
    env = _env(lv, lib, **kw)
    if placement is not None:
        env.set_placement(_dev(placement))
        env.reset()
    acts = _dev(bm.moves(name, agents, 5))
    for k in range(STEPS):
        r, d, sh = env.step(acts[k])
        ctx = "%s x%d %s %s step %d" % (name, agents, lib, policy, k)
        assert np.array_equal(r.cpu().numpy(), ref[k]["reward"]), ctx
        assert np.array_equal(d.cpu().numpy(), ref[k]["done"]), ctx
        assert np.array_equal(bits(sh.cpu().numpy()), bits(ref[k]["shaping"])), ctx
        hs = env.snapshot()
        assert (hs["error"] == 0).all(), ctx
        assert_snapshots_equal(hs, ref[k]["snapshot"], ctx)
    m = env.read_metrics()
    assert m["env_steps"] == N * STEPS and m["episodes"] == sum(int(s["done"].sum()) for s in ref)
    assert m["reward_sum"] == sum(int(s["reward"].sum()) for s in ref)


def _run_fused(name, lib, policy, monkeypatch, waves=0, lanes=1, dtype="int32", C=3, radius=2, blind=0):
    monkeypatch.setenv("OC_LAUNCH", policy)
    lv = bm.level(name, 2)
    ref = bm.fused_reference(name, C, radius, blind)
    env = _env(lv, lib, num_communication=C, fow_radius=radius, waves_per_64=waves, obs_dtype=DTYPES[dtype],
               partner_config={"BLIND": bool(blind & 2)}, ego_config={"BLIND": bool(blind & 1)})
    if waves:       # the launch taken (the generic library has no two-way split: one wave then)
        general = blind != 0
        assert env.launch_waves(general=general) == (1 if (lib == "generic" and waves == 2) else waves)
        assert env.launch_lanes(general=general) == lanes
    acts = _dev(bm.fused_actions(name, C))
    for k in range(STEPS):
        o, t, r, d = env.multi_step(acts[k])
        ctx = "%s %s %s waves=%d lanes=%d %s step %d" % (name, lib, policy, waves, lanes, dtype, k)
        assert o.dtype == DTYPES[dtype]
        assert np.array_equal(d.cpu().numpy(), ref[k]["done"]), ctx
        assert np.array_equal(o.cpu().numpy().astype(np.int64), ref[k]["obs"].astype(np.int64)), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(ref[k]["timestep"])), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ref[k]["reward"])), ctx
        assert np.array_equal(env.comm.cpu().numpy(), ref[k]["comm"]), ctx
        assert np.array_equal(env.reward.cpu().numpy(), ref[k]["sparse"]), ctx
        hs = env.snapshot()
        assert (hs["error"] == 0).all(), ctx
        assert_snapshots_equal(hs, ref[k]["snapshot"], ctx)
    m = env.read_metrics()
    assert m["env_steps"] == N * STEPS and m["episodes"] == sum(int(s["done"].sum()) for s in ref)
    return ref


# ---- seeded many-env runs ---------------------------------------------------------------------
BASE_MAPS = [("wide_16x8", 2), ("tall_8x16", 3), ("odd_13x9", 4)]
# (the generic library holds the base step on one wave only)
BASE_RUNS = [("generic", "step_split=1"), ("level", "step_split=1"), ("level", "step_split=2"),
             ("structure", "step_split=2"), ("structure", "step_split=1")]


@pytest.mark.parametrize("lib,policy", BASE_RUNS, ids=["%s-%s" % r for r in BASE_RUNS])
@pytest.mark.parametrize("name,agents", BASE_MAPS, ids=["%s-a%d" % c for c in BASE_MAPS])
def test_base_step_matches_oracle(monkeypatch, name, agents, lib, policy):
    _run_base(name, agents, lib, policy, monkeypatch)


# (waves per 64 envs, lanes per env); the lane split is the four-way split's, in the specialised libraries
LAUNCHES = [(1, 1), (2, 1), (4, 1), (4, 2)]
FUSED_RUNS = [("wide_16x8", lib, w, ln) for lib in LIBS for w, ln in LAUNCHES if not (lib == "generic" and ln == 2)]
FUSED_RUNS += [(name, lib, w, ln) for name in ("tall_8x16", "odd_13x9") for lib in LIBS
               for w, ln in ((1, 1), (4, 1 if lib == "generic" else 2))]


@pytest.mark.parametrize("name,lib,waves,lanes", FUSED_RUNS, ids=["%s-%s-w%d-l%d" % r for r in FUSED_RUNS])
def test_fused_step_matches_oracle(monkeypatch, name, lib, waves, lanes):
    _run_fused(name, lib, "lanes=%d" % lanes, monkeypatch, waves=waves, lanes=lanes)


@pytest.mark.parametrize("dtype", ["int8", "float32"])
def test_fused_step_row_types(monkeypatch, dtype):
    _run_fused("wide_16x8", "level", "lanes=1", monkeypatch, waves=4, lanes=1, dtype=dtype)


def test_64_cell_control_on_the_generic_library(monkeypatch):
    """8 x 8: the largest map on the one-word path, so that `nc > 64` is pinned from both sides."""
    lv = bm.level("control_8x8", 2)
    assert lv.width * lv.height == 64
    _run_base("control_8x8", 3, "generic", "step_split=1", monkeypatch)
    _run_fused("control_8x8", "generic", "lanes=1", monkeypatch, waves=1)


# ---- tables in LDS ----------------------------------------------------------------------------
def test_table_image_of_a_128_cell_map_is_16960_bytes():
    """128^2 distance bytes + 4 * 128 probe bytes + 64 Counter bytes = 1 060 uint4: with 64 threads the
    copy's four unrolled loads cover 256 of them, with 256 threads 1 024 -- the strided loop moves the
    rest (at 256 threads: uint4 1 024 .. 1 059 = bytes 16 384 .. 16 959, the probe and Counter tables)."""
    lv = bm.level("wide_16x8", 2)
    nc = lv.width * lv.height
    assert nc == 128 and ((nc * nc + 15) & ~15) + 4 * 128 + 64 == 16960 == 1060 * 16


LDS_POLICIES = ["lds=1", "lds=1,block=256"]


@pytest.mark.parametrize("policy", LDS_POLICIES)
@pytest.mark.parametrize("lib", ["generic", "level"])
def test_tables_in_lds_fused_step(monkeypatch, lib, policy):
    _run_fused("wide_16x8", lib, policy + ",split=1", monkeypatch)


@pytest.mark.parametrize("policy", LDS_POLICIES)
@pytest.mark.parametrize("name,agents,lib", [("wide_16x8", 2, "level"), ("tall_8x16", 3, "generic"),
                                             ("dup_16x8", 2, "generic"), ("dup_16x8", 2, "level")])
def test_tables_in_lds_base_step(monkeypatch, name, agents, lib, policy):
    """dup_16x8 repeats a type: its shaping terms read the per-cell probe table, the last 576 bytes of
    the image but 64."""
    if name == "dup_16x8":
        assert bm.level(name, agents).has_dup
    _run_base(name, agents, lib, policy + ",step_split=1", monkeypatch)


# ---- observation edges ------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["generic", "level"])
@pytest.mark.parametrize("radius", [0, 3, 1000])
def test_fog_radii_with_a_blind_partner(monkeypatch, radius, lib):
    """The general variant (a BLIND seat is no standard configuration): is_hidden and the encodings rows
    of both viewers.  At radius 3 on 16 x 8 the viewers see some items and not others."""
    ref = _run_fused("wide_16x8", lib, "lanes=1", monkeypatch, C=2, radius=radius, blind=2)
    M = bm.level("wide_16x8", 2).num_items
    assert M == 4                                                   # (rows 0..3 x, 4..7 y, 8..11 state, 12..15 is_hidden)
    hidden = np.stack([s["obs"][0, 12:16] for s in ref])            # the sighted ego's is_hidden rows
    blind = np.stack([s["obs"][1, 12:16] for s in ref])
    assert (blind == 1).all()
    if radius == 3:
        assert (hidden == 1).any() and (hidden == 0).any()
        ax = np.stack([s["snapshot"]["agents"][:, 0, 0] for s in ref])     # ... also from the far columns
        assert ((hidden == 0) & (ax[:, None, :] >= 12)).any() and ((hidden == 1) & (ax[:, None, :] >= 12)).any()
    elif radius == 1000:
        assert (hidden == 0).all()


# ---- image kernel -----------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["generic", "level"])
@pytest.mark.parametrize("name", ["wide_16x8", "tall_8x16", "square_11x11"])
def test_image_kernel_at_32_words_per_plane(monkeypatch, name, lib):
    from oracle import oracle
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    lv = bm.level(name, 2)
    cells = lv.width * lv.height
    q = (cells + 3) >> 2
    env = _env(lv, lib)
    words = env._L.oc_image_words(env._h)
    assert words == 7 * q and q == (32 if cells == 128 else 31)
    image, margin = with_margin(torch.zeros((2, words, N), dtype=torch.int32, device="cuda:0"))
    holding, hmargin = with_margin(torch.zeros((2, N), dtype=torch.int8, device="cuda:0"))
    ora = oracle.OracleBatch(lv.blob, N, threads=4)
    acts = bm.moves(name, 2, 5)
    acts_d = _dev(acts)
    fogged = seen = 0
    for k in range(40):
        env.step(acts_d[k])
        ora.step(acts[k], auto_reset=True)
        assert_snapshots_equal(env.snapshot(), ora.snapshot_all(), "%s step %d" % (name, k))
        if k % 8 != 7:
            continue
        for radius in (3, 0, 1000):
            env._call("oc_obs_image", env._h, env._p(env.state), radius, env._p(image), env._p(holding), N)
            b = image.cpu().numpy().view(np.uint8).reshape(2, 7, q, N, 4)       # little-endian bytes
            flat = np.moveaxis(b, 4, 3).reshape(2, 7, 4 * q, N).view(np.int8)
            mo, ho = ora.obs_image(radius)
            ctx = "%s %s step %d radius %d" % (name, lib, k, radius)
            assert (flat[:, :, cells:] == 0).all(), ctx
            got = flat[:, :, :cells].reshape(2, 7, lv.width, lv.height, N)
            if not np.array_equal(got, mo):
                v, p, x, y, i = (int(c) for c in np.argwhere(got != mo)[0])
                raise AssertionError("%s: viewer %d plane %d cell (%d, %d) env %d: %d, oracle %d"
                                     % (ctx, v, p, x, y, i, got[v, p, x, y, i], mo[v, p, x, y, i]))
            assert np.array_equal(holding.cpu().numpy().astype(np.int32), ho), ctx
            assert (margin == SENTINEL).all() and (hmargin == SENTINEL).all(), ctx
            if radius == 3:
                fogged += int((mo == -1).sum())
                seen += int((mo[:, 3:] > 0).sum())
    assert fogged > 0 and seen > 0


# ---- placement on many Counters ---------------------------------------------------------------
def _counter_cells(lv):
    return np.array([x | (y << 4) for x, y in lv.counters], np.int32)


def test_host_placements_use_every_counter(monkeypatch):
    lv = bm.level("random_16x8", 2)
    cc = _counter_cells(lv)
    nc, ns = len(cc), len(lv.scatter_items)
    assert lv.random_placement and nc == 49 and ns == 4 and lv.width * lv.height == 128
    place = np.zeros((lv.num_items, N), np.int32)
    for i in range(N):          # env i: Counters 4 i, 4 i + 1, ... (mod 49), dealt to the items in turn
        for k, item in enumerate(lv.scatter_items):
            place[item, i] = cc[(4 * i + (k + i) % ns) % nc]
    assert set(place.reshape(-1).tolist()) == set(cc.tolist())
    assert (place & 15).max() == 15 and (place >> 4).max() == 7        # the east wall and the south wall
    for lib, policy in (("generic", "step_split=1"), ("level", "step_split=2")):
        _run_base("random_16x8", 2, lib, policy, monkeypatch, placement=place)


@pytest.mark.parametrize("lib,policy", [("generic", "step_split=1"), ("level", "step_split=2"),
                                        ("level", "lds=1,step_split=1"), ("generic", "lds=1,block=256,step_split=1")])
def test_in_kernel_draw_matches_oracle_and_reaches_every_counter(monkeypatch, lib, policy):
    """placement_mode='rng': the drawn cells are read back after the reset and after every auto-reset and
    handed to the oracle, then the full state is compared.  Every drawn cell is a Counter, an env's four
    are distinct, and every one of the 49 Counters is drawn: an env-reset draws 4 of 49 without
    replacement, so it misses a given Counter with probability 45 / 49; the run makes at least
    229 * (1 + 4) = 1 145 env-resets, and (45 / 49)^1145 = exp(-97.5) is far below 1e-9 (244 resets
    would do)."""
    from oracle import oracle
    monkeypatch.setenv("OC_LAUNCH", policy)
    name = "random_16x8"
    lv = bm.level(name, 2)
    cc = _counter_cells(lv)
    assert len(cc) == 49 and (45.0 / 49.0) ** (N * (1 + STEPS // bm.T)) < 1e-9
    env = _env(lv, lib, placement_mode="rng", seed=17)
    ora = oracle.OracleBatch(lv.blob, N, threads=4)
    acts = bm.moves(name, 2, 5)
    acts_d = _dev(acts)

    def drawn(mask):
        cells = (env.state[env.A:env.A + env.M].cpu().numpy() & 255).astype(np.int32)
        sub = cells[:, mask]
        assert np.isin(sub, cc).all()
        assert all(len(set(sub[:, j].tolist())) == env.M for j in range(sub.shape[1]))
        return cells, np.bincount(np.searchsorted(np.sort(cc), sub.reshape(-1)), minlength=len(cc))

    cells, hist = drawn(np.ones(N, bool))
    ora.set_placement(cells)
    ora.reset()
    assert_snapshots_equal(env.snapshot(), ora.snapshot_all(), "after reset")
    resets = N
    for k in range(STEPS):
        ctx = "%s %s step %d" % (lib, policy, k)
        r, d, sh = env.step(acts_d[k])
        ro, do, sho = ora.step(acts[k], auto_reset=False)
        dn = d.cpu().numpy()
        assert np.array_equal(dn, do) and np.array_equal(r.cpu().numpy(), ro), ctx
        assert np.array_equal(bits(sh.cpu().numpy()), bits(sho)), ctx
        if dn.any():
            cells, h = drawn(dn != 0)
            hist += h
            ora.set_placement(cells)
            ora.reset(dn)
            resets += int(dn.sum())
        hs, os_ = env.snapshot(), ora.snapshot_all()
        assert (hs["error"] == 0).all() and (os_["error"] == 0).all(), ctx
        assert_snapshots_equal(hs, os_, ctx)
    assert resets >= N * (1 + STEPS // bm.T)
    assert (hist > 0).all(), "Counters never drawn: %s" % [lv.counters[i] for i in np.nonzero(hist == 0)[0]]


# ---- map sets ---------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
def test_map_set_of_two_maps_above_64_cells(monkeypatch, waves):
    from gym_comm_amd.batched import BatchedOvercooked
    from test_mapset_gpu import C, RADIUS, SetOracle
    monkeypatch.delenv("OC_LAUNCH", raising=False)
    lvs = [bm.level("wide_16x8", 2), bm.level("variant_12x10", 2)]
    assert all(lv.width * lv.height > 64 for lv in lvs)
    gm = (0, 1, 1, 0)
    env = BatchedOvercooked.from_maps(lvs, group_map=list(gm), num_envs=N, device="cuda:0", num_communication=C,
                                      fow_radius=RADIUS, auto_reset=True, waves_per_64=waves)
    assert env._L.oc_is_specialized() == 1 and env.launch_waves() == waves
    ora = SetOracle(lvs, gm, N)
    ora.reset()
    acts = bm.fused_actions("wide_16x8", C)
    acts_d = _dev(acts)
    far = [False, False]
    for k in range(STEPS):
        o, t, r, d = env.multi_step(acts_d[k])
        ref = ora.multi_step(acts[k])
        ctx = "waves=%d step %d" % (waves, k)
        assert np.array_equal(d.cpu().numpy(), ref["done"]), ctx
        assert np.array_equal(o.cpu().numpy(), ref["obs"]), ctx
        assert np.array_equal(bits(t.cpu().numpy()), bits(ref["timestep"])), ctx
        assert np.array_equal(bits(r.cpu().numpy()), bits(ref["reward"])), ctx
        assert np.array_equal(env.comm.cpu().numpy(), ref["comm"]), ctx
        assert np.array_equal(env.reward.cpu().numpy(), ref["sparse"]), ctx
        assert_snapshots_equal(env.snapshot(), ref["snapshot"], ctx)
        for m, lv in enumerate(lvs):
            far[m] |= bool((ref["snapshot"]["agents"][ora.idx[m], :, 0] >= lv.width - 2).any())
    assert far == [True, True]
    got = env.read_metrics()
    assert got["env_steps"] == N * STEPS and [p["env_steps"] for p in got["per_map"]] == [
        STEPS * len(ora.idx[0]), STEPS * len(ora.idx[1])]
