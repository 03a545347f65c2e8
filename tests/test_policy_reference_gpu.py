"""The fused MLP policy (csrc/oc_policy.hip, and its copy inside the step kernel) env by env
against the float64 restatement in tests/policy_ref.py.

Logits must lie within policy_ref.logit_bound of the emulated reference (the header's roundings
and nothing else); greedy actions are the first maximum; sampled actions are the fp64 inverse CDF
of the host PCG32 draw, and the streams advance bit for bit.  Each comparison proves it can fail:
planted mutations of the reference (a feature, the timestep, a comm row, the b2 fold, the
activation, the draw) must be rejected on the same data.  The inputs are synthetic observation
rows [F][n] whose features differ from env to env and reach the ends of each element type."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import policy_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

ODT = {"int32": torch.int32, "int8": torch.int8, "float32": torch.float32}
WORST = {"ratio": 0.0}          # largest |kernel - reference| / bound seen in this session


def _policy(F, C, seed, scale):
    """MLPPolicy(seed) with its first layer re-drawn for F features (same init rule), every
    weight scaled by `scale`."""
    from gym_comm_amd.vec_env import MLPPolicy
    pol = MLPPolicy(3, C, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        pol.w1 = torch.nn.Parameter((torch.rand((64, F), generator=g) * 2 - 1) / float(np.sqrt(F)))
        for t in (pol.w1, pol.b1, pol.wt, pol.w2, pol.b2):
            t.mul_(scale)
    return pol.cuda()


def _weights(pol):
    return tuple(t.detach().cpu().numpy().astype(np.float64) for t in (pol.w1, pol.wt, pol.b1, pol.w2, pol.b2))


def _rows(F, n, odt, seed):
    """Mostly small values (as observations are), one element in ten drawn from the type's whole
    range (int8 -128..127, int32 +-2048, float32 +-2048 with values fp16 cannot hold), and both
    ends of the range present."""
    rng = np.random.default_rng(seed)
    if odt == "float32":
        small = rng.uniform(-2, 2, (F, n))
        big = rng.uniform(-2048, 2048, (F, n))
        lo, hi = -2047.7, 2047.3
    else:
        lo, hi = (-128, 127) if odt == "int8" else (-2048, 2048)
        small = rng.integers(-2, 3, (F, n))
        big = rng.integers(lo, hi + 1, (F, n))
    x = np.where(rng.random((F, n)) < 0.1, big, small)
    x.flat[0] = lo
    x.flat[-1] = hi
    return torch.from_numpy(x.astype({"int32": np.int32, "int8": np.int8, "float32": np.float32}[odt])).cuda()


def _timesteps(n, T, seed):
    t = np.random.default_rng(seed + 7).integers(0, T + 1, n)
    return torch.from_numpy(t / float(T)).cuda()


def _check_logits(got, w, rows, ts, tag=""):
    """|kernel - emulated reference| <= bound everywhere; returns (reference, bound)."""
    ref = pr.ref_logits(*w, rows, ts)
    bound, _ = pr.logit_bound(*w, rows, ts)
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-30)).max())
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print("policy-ref %s: max err %.3g, max bound %.3g, max err/bound %.3f (session max %.3f)"
          % (tag, err.max(), bound.max(), ratio, WORST["ratio"]))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (tag, bad[:5].tolist(), err[tuple(bad[0])], bound[tuple(bad[0])])
    return ref, bound


def _mutants(w, rows, ts, C):
    """Planted bugs, each as the logits the reference would produce with it."""
    w1, wt, b1, w2, b2 = w
    F, n = rows.shape
    out = {}
    if F >= 9:          # two features across the 8-feature half-k-step boundary
        sw = rows.copy()
        sw[[7, 8]] = sw[[8, 7]]
        out["features 7/8 swapped"] = pr.ref_logits(w1, wt, b1, w2, b2, sw, ts)
    out["timestep and bias swapped"] = pr.ref_logits(w1, b1, wt, w2, b2, rows, ts)
    out["timestep of env i+1"] = pr.ref_logits(w1, wt, b1, w2, b2, rows, np.roll(ts, -1))
    out["timestep of env i-1"] = pr.ref_logits(w1, wt, b1, w2, b2, rows, np.roll(ts, 1))
    ref = pr.ref_logits(w1, wt, b1, w2, b2, rows, ts)
    space = np.zeros((32, n))          # the second product's 32 rows (padding rows are 0)
    space[0:4] = ref[0:4]
    for c in range(C):
        space[pr.comm_row(c)] = ref[4 + c]
    for d in (4, -4):
        m = ref.copy()
        for c in range(C):
            m[4 + c] = space[(pr.comm_row(c) + d) % 32]
        out["comm row %+d" % d] = m
    out["b2 without the row-sum fold"] = pr.ref_logits(w1, wt, b1, w2, b2, rows, ts, fold=False)
    out["tanh replaced by r"] = pr.ref_logits(w1, wt, b1, w2, b2, rows, ts, act="r")
    return out


def _assert_mutants_fail(got, w, rows, ts, C, bound):
    for name, m in _mutants(w, rows, ts, C).items():
        assert (np.abs(got - m) > bound).any(), "the bound lets a planted bug through: " + name


# (F, C, obs type, n, players, OC_POLICY_WG32, weight scale, T): every F is one to five k-steps
# and every (F + 2) mod 16 edge; every C reaches a comm-row group edge; two players always with
# padding workgroups between their ranges (gx8 > gx)
SWEEP = [
    (1, 1, "int8", 1, 1, 0, 1, 333),
    (14, 3, "int32", 31, 2, 1, 4, 500),
    (15, 4, "float32", 32, 1, 0, 32, 333),
    (16, 5, "int8", 33, 2, 0, 4, 500),
    (29, 8, "int32", 64, 1, 1, 1, 333),
    (30, 9, "float32", 65, 2, 0, 4, 500),
    (31, 12, "int8", 777, 1, 0, 32, 333),
    (46, 16, "int32", 4129, 2, 1, 4, 500),
    (47, 1, "float32", 777, 2, 1, 1, 333),
    (62, 4, "int8", 4129, 1, 1, 4, 500),
    (63, 16, "float32", 33, 1, 0, 4, 333),
    (78, 9, "int32", 65, 2, 1, 32, 500),
    (30, 12, "int8", 64, 2, 1, 1, 500),
    (46, 8, "float32", 31, 1, 1, 32, 333),
    (14, 5, "int32", 777, 1, 0, 1, 500),
    (78, 3, "float32", 4129, 2, 0, 1, 333),
]


@pytest.mark.parametrize("F,C,odt,n,players,wg32,scale,T", SWEEP,
                         ids=["F%d-C%d-%s-n%d-p%d-wg%d-x%d" % (c[0], c[1], c[2], c[3], c[4], 32 if c[5] else 64, c[6])
                              for c in SWEEP])
def test_logits_and_greedy_actions_match_the_float64_reference(F, C, odt, n, players, wg32, scale, T, monkeypatch):
    from gym_comm_amd.vec_env import FusedMLPPartner
    if wg32:
        monkeypatch.setenv("OC_POLICY_WG32", "1")
    else:
        monkeypatch.delenv("OC_POLICY_WG32", raising=False)
    pols = [_policy(F, C, 20 + 7 * k + F, scale) for k in range(players)]
    rows = [_rows(F, n, odt, 100 * F + C + k) for k in range(players)]
    ts = _timesteps(n, T, F + n)
    fused = [FusedMLPPartner(p, sample=False, keep_logits=True) for p in pols]
    FusedMLPPartner.launch(fused, rows, ts)
    torch.cuda.synchronize()
    tsn = ts.cpu().numpy()
    for k in range(players):
        w, x = _weights(pols[k]), rows[k].cpu().numpy()
        got = fused[k].logits.cpu().numpy().astype(np.float64)
        pairs = fused[k].pairs.cpu().numpy()
        ref, bound = _check_logits(got, w, x, tsn, "F%d C%d %s n%d player %d" % (F, C, odt, n, k))
        if n >= 32 and scale < 32:
            # (at x32 nearly every hidden unit saturates: a wrong timestep changes nothing measurable)
            _assert_mutants_fail(got, w, x, tsn, C, bound)
        if scale == 4 and odt != "float32":
            # the module's own accuracy claim at x4 on the small features (|x| <= 2)
            small = (np.abs(x) <= 2).all(axis=0)
            exact = pr.ref_logits(*w, x, tsn, emulate=False)
            assert np.abs(got - exact)[:, small].max(initial=0) < 2e-2
        for lo, hi, col in ((0, 4, 0), (4, 4 + C, 1)):
            # greedy = the first maximum of the kernel's own logits, exactly ...
            assert np.array_equal(pairs[:, col], pr.first_argmax(got[lo:hi]))
            # ... and the reference's argmax wherever its top-2 gap is beyond the bound
            blk = ref[lo:hi]
            if hi - lo > 1:
                top2 = np.sort(blk, axis=0)[-2:]
                clear = (top2[1] - top2[0]) > 2 * bound[lo:hi].max(axis=0)
            else:
                clear = np.ones(n, bool)
            assert np.array_equal(pairs[clear, col], pr.first_argmax(blk)[clear])


def test_real_observations_at_x4_stay_within_2e_2_of_the_exact_module():
    """The accuracy claim of include/oc_policy.h (logits within 2e-2 of the fp32 module) on the
    observation rows a stepped env leaves, with the default init scaled x4, for all three
    element types -- and within the tight bound of the emulated reference."""
    from gym_comm_amd.batched import BatchedOvercooked
    from gym_comm_amd.vec_env import FusedMLPPartner, MLPPolicy
    for level, C, odt, n in (("full-divider_salad", 4, torch.int8, 1000), ("open-divider_tl", 9, torch.float32, 777),
                             ("open-divider_tomato", 1, torch.int32, 2048)):
        env = BatchedOvercooked(level, num_agents=2, num_envs=n, max_num_timesteps=60, num_communication=C,
                                communication_on=True, fow_radius=2, obs_dtype=odt, auto_reset=True)
        g = torch.Generator(device="cuda").manual_seed(4)
        hi = torch.tensor([4, C, 4, C], device="cuda").view(4, 1)
        for _ in range(20):
            env.multi_step((torch.rand((4, n), generator=g, device="cuda") * hi).to(torch.int32))
        pol = MLPPolicy(env.S, C, seed=31).cuda()
        with torch.no_grad():
            for t in (pol.w1, pol.b1, pol.wt, pol.w2, pol.b2):
                t.mul_(4)
        fused = FusedMLPPartner(pol, sample=False, keep_logits=True)
        FusedMLPPartner.launch([fused], [env.obs[1]], env.timestep)
        got = fused.logits.cpu().numpy().astype(np.float64)
        w, x, ts = _weights(pol), env.obs[1].cpu().numpy(), env.timestep.cpu().numpy()
        _check_logits(got, w, x, ts, "%s C%d real obs x4" % (level, C))
        err = np.abs(got - pr.ref_logits(*w, x, ts, emulate=False)).max()
        print("policy-ref %s: x4 module error %.3g" % (level, err))
        assert err < 2e-2


def test_nothing_is_written_past_n(monkeypatch):
    """pairs / rng / logits as views at the front of larger buffers: the tails keep their
    sentinel (two players, padding workgroups, a ragged last wave; both workgroup mappings)."""
    from gym_comm_amd import _lib
    from gym_comm_amd.vec_env import FusedMLPPartner
    L = _lib.load(lib="policy")
    F, C, n, tail = 33, 6, 777, 4096
    SENT = -0x5A5A5A5B
    ts = _timesteps(n, 333, 1)
    for wg32 in ("0", "1"):
        monkeypatch.setenv("OC_POLICY_WG32", wg32)
        players, keep = [], []
        for k in range(2):
            pol = _policy(F, C, 60 + k, 4)
            fz = FusedMLPPartner(pol, sample=True, seed=3 + k)       # for its packed weights
            rows = _rows(F, n, "int32", 9 + k)
            pairs = torch.full((2 * n + tail,), SENT, dtype=torch.int32, device="cuda")
            rng = torch.full((2 * n + tail,), SENT, dtype=torch.int32, device="cuda")
            rng[:2 * n] = torch.arange(2 * n, dtype=torch.int32, device="cuda") * 7919
            logits = torch.full(((4 + C) * n + tail,), float("nan"), dtype=torch.float32, device="cuda")
            players.append(_lib.PolicyPlayer(rows.data_ptr(), fz._w[0].data_ptr(), fz._w[1].data_ptr(),
                                             fz._w[2].data_ptr(), rng.data_ptr(), pairs.data_ptr(),
                                             logits.data_ptr()))
            keep.append((fz, rows, pairs, rng, logits, pol))
        arr = (_lib.PolicyPlayer * 2)(*players)
        rc = L.oc_policy_mlp(arr, 2, ts.data_ptr(), F, C, 0, n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.oc_policy_last_error()
        torch.cuda.synchronize()
        for fz, rows, pairs, rng, logits, pol in keep:
            assert (pairs[2 * n:] == SENT).all() and (rng[2 * n:] == SENT).all()
            assert torch.isnan(logits[(4 + C) * n:]).all()
            assert not torch.isnan(logits[:(4 + C) * n]).any()
            s_new, _ = pr.pcg32(np.arange(2 * n, dtype=np.int64) * 7919)
            assert np.array_equal(s_new.astype(np.uint32), rng[:2 * n].cpu().numpy().view(np.uint32))
            pv = pairs[:2 * n].view(n, 2)
            assert (pv[:, 0] >= 0).all() and (pv[:, 0] < 4).all() and (pv[:, 1] >= 0).all() and (pv[:, 1] < C).all()
            _check_logits(logits[:(4 + C) * n].view(4 + C, n).cpu().numpy().astype(np.float64), _weights(pol),
                          rows.cpu().numpy(), ts.cpu().numpy(), "guarded wg32=%s" % wg32)


def test_greedy_ties_pick_the_first_index():
    """Zero weights and tied biases: every logit of a head is the same fp32 value in every env,
    and the greedy rule (torch.argmax's) takes the first maximum."""
    from gym_comm_amd.vec_env import FusedMLPPartner
    for C, n in ((4, 777), (12, 65)):
        pol = _policy(29, C, 5, 1)
        with torch.no_grad():
            for t in (pol.w1, pol.wt, pol.b1, pol.w2):
                t.zero_()
            b = [1.0, 1.0, 0.0, 1.0] + [0.5] * C
            b[4] = -0.25              # a lower first comm logit: the first of the tied maxima is comm 1
            pol.b2.copy_(torch.tensor(b).view(-1, 1))
        fused = FusedMLPPartner(pol, sample=False, keep_logits=True)
        FusedMLPPartner.launch([fused], [_rows(29, n, "int8", 3)], _timesteps(n, 500, 3))
        assert (fused.pairs[:, 0] == 0).all() and (fused.pairs[:, 1] == 1).all()
        lg = fused.logits
        assert (lg[0] == lg[1]).all() and (lg[1] == lg[3]).all() and (lg[5:] == lg[5]).all()


def _draw_mutants(st0):
    """Uniforms of planted sampler bugs: the streams swapped, the draw taken from the state
    before the advance, the neighbour env's draw."""
    _, out = pr.pcg32(st0)
    s = np.asarray(st0).astype(np.int64) & 0xFFFFFFFF          # the state one draw back, so that
    back = ((s - pr.PCG_INC) * pow(pr.PCG_MULT, -1, 1 << 32)) & 0xFFFFFFFF   # its advance IS st0
    _, pre = pr.pcg32(back)
    return {"streams swapped": pr.draw_u(out)[::-1], "draw before the advance": pr.draw_u(pre),
            "neighbour env's draw": np.roll(pr.draw_u(out), 1, axis=1)}


def _check_samples(pairs, got, st0, st1, w, rows, ts, C, tag, stats):
    """One sampled launch of one player, env by env."""
    s_new, out = pr.pcg32(st0)
    assert np.array_equal(s_new.astype(np.uint32), st1.view(np.uint32)), tag     # row 0 move, row 1 comm
    u = pr.draw_u(out)
    ref = pr.ref_logits(*w, rows, ts)
    bound, _ = pr.logit_bound(*w, rows, ts)
    muts = _draw_mutants(st0)
    caught = {k: 0 for k in muts}
    for lo, hi, col, row in ((0, 4, 0, 0), (4, 4 + C, 1, 1)):
        own, margin = pr.ref_sample(got[lo:hi] / pr.LN2, u[row])
        ok = margin >= 1e-5
        stats["pairs"] += ok.size
        stats["excluded"] += int((~ok).sum())
        assert np.array_equal(pairs[ok, col], own[ok]), (tag, col, np.argwhere(pairs[ok, col] != own[ok])[:5])
        exp, rmargin = pr.ref_sample(ref[lo:hi] / pr.LN2, u[row])
        clear = rmargin > 2 * bound[lo:hi].max(axis=0) + 1e-5
        stats["ref_pairs"] += clear.size
        stats["ref_excluded"] += int((~clear).sum())
        assert np.array_equal(pairs[clear, col], exp[clear]), (tag, col)
        for name, um in muts.items():
            a, m = pr.ref_sample(got[lo:hi] / pr.LN2, um[row])
            caught[name] += int((pairs[m >= 1e-5, col] != a[m >= 1e-5]).sum())
    for name, cnt in caught.items():
        assert cnt > 0, "a planted sampler bug passes: " + name


@pytest.mark.parametrize("F,C,odt,n,players,wg32,scale", [(30, 9, "int8", 777, 2, 0, 4),
                                                          (47, 16, "float32", 4129, 1, 1, 1),
                                                          (14, 1, "int32", 65, 2, 1, 4),
                                                          (29, 4, "int32", 2048, 1, 0, 1)],
                         ids=["F30-C9-int8-p2", "F47-C16-float32-wg32", "F14-C1-int32-p2-wg32", "F29-C4-int32"])
def test_sampled_actions_and_streams_match_the_host_pcg32_env_by_env(F, C, odt, n, players, wg32, scale, monkeypatch):
    from gym_comm_amd.vec_env import FusedMLPPartner
    if wg32:
        monkeypatch.setenv("OC_POLICY_WG32", "1")
    else:
        monkeypatch.delenv("OC_POLICY_WG32", raising=False)
    pols = [_policy(F, C, 40 + k, scale) for k in range(players)]
    rows = [_rows(F, n, odt, 300 + k) for k in range(players)]
    ts = _timesteps(n, 333, 5)
    fused = [FusedMLPPartner(p, sample=True, seed=70 + k, keep_logits=True) for k, p in enumerate(pols)]
    stats = dict(pairs=0, excluded=0, ref_pairs=0, ref_excluded=0)
    tsn = ts.cpu().numpy()
    for launch in range(3):
        for f in fused:
            f._buffers(n)
        st0 = [f._rng.cpu().numpy().copy() for f in fused]
        FusedMLPPartner.launch(fused, rows, ts)
        for k, f in enumerate(fused):
            _check_samples(f.pairs.cpu().numpy(), f.logits.cpu().numpy().astype(np.float64), st0[k],
                           f._rng.cpu().numpy(), _weights(pols[k]), rows[k].cpu().numpy(), tsn, C,
                           "launch %d player %d" % (launch, k), stats)
    frac = stats["excluded"] / stats["pairs"]
    print("policy-ref sampling F%d C%d: %d of %d (env, head) draws excluded (%.4f %%); %d of %d not clear of the "
          "logit bound" % (F, C, stats["excluded"], stats["pairs"], 100 * frac, stats["ref_excluded"], stats["ref_pairs"]))
    assert frac <= 0.005


def test_sampling_with_huge_logit_spreads_takes_the_argmax():
    """Spreads of more than 200 between the top logit and the next: 2^x underflows to 0 for every
    other candidate, and the sample is the argmax in every env (and the streams still advance)."""
    from gym_comm_amd.vec_env import FusedMLPPartner
    F, C, n = 31, 5, 4129
    pol = _policy(F, C, 8, 1)
    with torch.no_grad():
        # saturated hidden units (r in {0, 1}) and a second layer whose logits are hundreds apart
        pol.w1.mul_(64)
        pol.w2.mul_(2000)
    rows = _rows(F, n, "int8", 12)
    ts = _timesteps(n, 500, 12)
    fused = FusedMLPPartner(pol, sample=True, seed=2, keep_logits=True)
    fused._buffers(n)
    wide_total = 0
    for _ in range(3):
        st0 = fused._rng.cpu().numpy().copy()
        FusedMLPPartner.launch([fused], [rows], ts)
        got = fused.logits.cpu().numpy().astype(np.float64)
        pairs = fused.pairs.cpu().numpy()
        s_new, _ = pr.pcg32(st0)
        assert np.array_equal(s_new.astype(np.uint32), fused._rng.cpu().numpy().view(np.uint32))
        for lo, hi, col in ((0, 4, 0), (4, 4 + C, 1)):
            top2 = np.sort(got[lo:hi], axis=0)[-2:]
            wide = (top2[1] - top2[0]) > 200
            wide_total += int(wide.sum())
            assert np.array_equal(pairs[wide, col], pr.first_argmax(got[lo:hi])[wide])
    assert wide_total > 0.5 * 3 * 2 * n, wide_total


def test_largest_batch_one_policy_call_can_address():
    """int8 rows with F * n just below 2^31 (the launcher's limit: 32-bit element offsets): the
    last 64 envs and a strided sample against the reference, logits, samples and streams."""
    from gym_comm_amd.vec_env import FusedMLPPartner
    F, C = 29, 1
    n = (2 ** 31 - 1) // F
    assert F * n < 2 ** 31 and F * (n + 1) >= 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.randint(-128, 128, (F, n), generator=g, device="cuda", dtype=torch.int8)
    ts = (torch.randint(0, 501, (n,), generator=g, device="cuda", dtype=torch.int32).double() / 500.0)
    pol = _policy(F, C, 77, 1)
    fused = FusedMLPPartner(pol, sample=True, seed=4, keep_logits=True)
    fused._buffers(n)
    idx = torch.cat([torch.arange(0, n - 64, 999_983, device="cuda"), torch.arange(n - 64, n, device="cuda")])
    st0 = fused._rng[:, idx].cpu().numpy()
    FusedMLPPartner.launch([fused], [rows], ts)
    got = fused.logits[:, idx].cpu().numpy().astype(np.float64)
    x = rows[:, idx].cpu().numpy()
    tsn = ts[idx].cpu().numpy()
    w = _weights(pol)
    _check_logits(got, w, x, tsn, "F*n = 2^31 - %d" % (2 ** 31 - F * n))
    stats = dict(pairs=0, excluded=0, ref_pairs=0, ref_excluded=0)
    _check_samples(fused.pairs[idx].cpu().numpy(), got, st0, fused._rng[:, idx].cpu().numpy(), w, x, tsn, C,
                   "largest batch", stats)
    assert stats["excluded"] <= 0.005 * stats["pairs"] + 1
    del rows, fused
    torch.cuda.empty_cache()


# the fused step kernel's copy of the policy (oc_step_opts.policy): the pairs it leaves for the
# next step against the reference on the observation rows and timestep that step wrote
STEP_CASES = [("open-divider_tomato", 1, "int32", 1500, True),      # F 27
              ("open-divider_tl", 1, "int8", 40000, True),          # F 30: two full k-steps
              ("open-divider_tomato", 4, "float32", 1500, False),   # F 33
              ("full-divider_salad", 4, "int8", 1500, True),        # F 39
              ("full-divider_salad", 4, "int32", 40000, False),
              ("open-divider_tl", 1, "float32", 1500, False),
              ("open-divider_tomato", 4, "int8", 40000, True)]


@pytest.mark.parametrize("level,C,odt,n,sample", STEP_CASES,
                         ids=["%s-C%d-%s-n%d-%s" % (c[0].split("_")[1], c[1], c[2], c[3], "sampled" if c[4] else "greedy")
                              for c in STEP_CASES])
def test_policy_inside_the_step_kernel_matches_the_reference(level, C, odt, n, sample):
    from types import SimpleNamespace
    from gym_comm_amd.vec_env import FusedMLPPartner, OvercookedVecEnv
    arg = SimpleNamespace(level=level, num_agents=2, max_num_timesteps=40, ego_config={}, partner_config={},
                          num_communication=C, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, n, seed=1, obs_dtype=ODT[odt])
    if venv._b.kernel_flavour != "spec":
        pytest.skip("the fused policies are built into the specialised libraries only (OC_SPECIALIZE=0 forces the generic one)")
    F = 22 + venv._b.S + 2 * C
    pols = [_policy(F, C, 90 + k, 4) for k in range(2)]
    ego = FusedMLPPartner(pols[0], sample=sample, seed=11)
    venv.partner = alt = FusedMLPPartner(pols[1], sample=sample, seed=12)
    venv.reset_tensors()
    loop = venv.closed_loop(ego, graph=False, one_launch=True)
    assert loop.one_launch
    checked = excluded = 0
    for step in range(4):
        before = [p._rng.cpu().numpy().copy() for p in (ego, alt)]
        loop.step()
        ts = venv._obs_tensors(0).timestep.cpu().numpy()
        for v, p in enumerate((ego, alt)):
            rows = venv._obs_tensors(v).rows.cpu().numpy()
            pairs = p.pairs.cpu().numpy()
            w = _weights(pols[v])
            ref = pr.ref_logits(*w, rows, ts)
            bound, _ = pr.logit_bound(*w, rows, ts)
            if sample:
                s_new, out = pr.pcg32(before[v])
                assert np.array_equal(s_new.astype(np.uint32), p._rng.cpu().numpy().view(np.uint32)), (step, v)
                u = pr.draw_u(out)
            for lo, hi, col in ((0, 4, 0), (4, 4 + C, 1)):
                blk = ref[lo:hi]
                if sample:
                    exp, margin = pr.ref_sample(blk / pr.LN2, u[col])
                    clear = margin > 2 * bound[lo:hi].max(axis=0) + 1e-5
                else:
                    exp = pr.first_argmax(blk)
                    top2 = np.sort(blk, axis=0)[-2:] if hi - lo > 1 else None
                    clear = ((top2[1] - top2[0]) > 2 * bound[lo:hi].max(axis=0) if top2 is not None
                             else np.ones(n, bool))
                checked += clear.size
                excluded += int((~clear).sum())
                assert np.array_equal(pairs[clear, col], exp[clear]), (step, v, col, np.argwhere(pairs[clear, col] != exp[clear])[:5])
    print("policy-ref step kernel %s C%d %s n%d: %d of %d (env, head) actions not clear of the bound"
          % (level, C, odt, n, excluded, checked))
    assert excluded <= 0.01 * checked
