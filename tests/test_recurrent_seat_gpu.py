"""-m gpu: the recurrent seat (include/oc_policy.h, last section: oc_policy_lstm_ac; ``FusedRecurrentPartner``)
env by env against tests/recurrent_ref.py.

One step from a random state: logits, value, h and c inside the derived bounds, element by element, with
bounds tight enough that six planted mutants of the reference are rejected on the same data; the mask; the
stores (nothing past n, state in place, state unwritten); envs independent of their batch; the tail
(sampler, greedy, ``score``, the -inf rule); and the seat in the env, eager and captured, step by step.

Against the PLAIN float32 module (recurrent_ref.step(emulate=False), each step from the kernel's own
previous state) the largest difference over the 60-step trajectory of the env test was measured on an
MI355X: logits 1.48e-3, value 1.34e-3 (weights at 4 x the init scale).  ``PLAIN_LOGITS`` / ``PLAIN_VALUE`` hold
those figures; the test asserts twice them -- a regression guard, not a claim."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import policy_ref as pr  # noqa: E402
import recurrent_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

OT = {"int32": 0, "int8": 1, "float32": 2}
SENT = -0x5A5A5A5B
GUARD = 257
PLAIN_LOGITS, PLAIN_VALUE = 1.48e-3, 1.34e-3
WORST = {}          # largest |kernel - reference| / bound seen in this session, per quantity


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _i32(k):
    return torch.full((k + GUARD,), SENT, dtype=torch.int32, device="cuda")


def _f32(k):
    return torch.full((k + GUARD,), float("nan"), dtype=torch.float32, device="cuda")


class Bufs:
    """The outputs of one raw launch for n envs: each a view at the front of a larger buffer whose tail keeps
    a canary (an int pattern; NaN for floats, which no output of a finite step is)."""

    def __init__(self, n, C):
        self.n, self.C = n, C
        self.pairs, self.move, self.comm, self.rng = _i32(2 * n), _i32(n), _i32(n), _i32(2 * n)
        self.log_prob, self.value, self.logits = _f32(n), _f32(n), _f32((4 + C) * n)
        self.h, self.c = _f32(64 * n), _f32(64 * n)

    def guards_intact(self, state=True, rng=True, finite=True):
        n, C = self.n, self.C
        for t, k in ((self.pairs, 2 * n), (self.move, n), (self.comm, n), (self.rng, 2 * n)):
            assert (t[k:] == SENT).all()
        if not rng:
            assert (self.rng == SENT).all()
        floats = [(self.log_prob, n), (self.value, n), (self.logits, (4 + C) * n)] + ([(self.h, 64 * n), (self.c, 64 * n)] if state else [])
        for t, k in floats:
            assert torch.isnan(t[k:]).all()
            if finite:
                assert not torch.isnan(t[:k]).any()
        if not state:
            assert torch.isnan(self.h).all() and torch.isnan(self.c).all()

    def out(self):
        """numpy views of the n envs' results."""
        n, C = self.n, self.C
        g = lambda t, k, shape: t[:k].reshape(shape).cpu().numpy()  # noqa: E731
        return SimpleNamespace(pairs=g(self.pairs, 2 * n, (n, 2)), move=g(self.move, n, (n,)), comm=g(self.comm, n, (n,)),
                               rng=g(self.rng, 2 * n, (2, n)), log_prob=g(self.log_prob, n, (n,)), value=g(self.value, n, (n,)),
                               logits=g(self.logits, (4 + C) * n, (4 + C, n)), h=g(self.h, 64 * n, (64, n)),
                               c=g(self.c, 64 * n, (64, n)))


def _guarded(a):
    """A float32 array as a device tensor at the front of a canary-tailed buffer."""
    t = _f32(a.size)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    return t


class Case:
    """A module, its packed images and inputs for n envs."""

    def __init__(self, F, C, odt, n, scale, seed=0, pol=None):
        from gym_comm_amd.vec_env import FusedRecurrentPartner
        self.F, self.C, self.odt, self.n = F, C, odt, n
        self.pol = pol if pol is not None else rr.make_module(F, C, 20 + F + seed, scale)
        self.w = rr.weights(self.pol)
        self.seat = FusedRecurrentPartner(self.pol.cuda(), sample=True, seed=70 + seed)
        self.rows_np = rr.make_rows(F, n, odt, 100 * F + C + n + seed)
        self.ts_np = np.random.default_rng(F + n + seed).integers(0, 334, n) / 333.0
        self.h_np, self.c_np, self.es_np = rr.make_state(n, F + n + seed)
        self.rows, self.ts = torch.from_numpy(self.rows_np).cuda(), torch.from_numpy(self.ts_np).cuda()
        from gym_comm_amd.batched import pcg32_seed_states
        self.rng0 = pcg32_seed_states(70 + seed, (2, n), "cuda")

    def launch(self, b, h=None, c=None, es="own", rng=True, given=None, alias=False, write_state=True, rows=None, ts=None,
               rng0=None, n=None):
        """One raw launch into ``b``.  h, c: numpy [64][n] (default: the case's); es: numpy [n], "own" or None
        (a NULL pointer).  alias: the state is updated in place, in ``b.h`` / ``b.c``.  Returns the state-in
        tensors (kept alive; after an aliased launch they ARE b.h / b.c)."""
        from gym_comm_amd import _lib
        L = _lib.load(lib="policy")
        n = self.n if n is None else n
        h = self.h_np if h is None else h
        c = self.c_np if c is None else c
        es = self.es_np if isinstance(es, str) else es
        if alias:
            b.h[:64 * n], b.c[:64 * n] = torch.from_numpy(h.reshape(-1)).cuda(), torch.from_numpy(c.reshape(-1)).cuda()
            hin, cin = b.h, b.c
        else:
            hin, cin = _guarded(h), _guarded(c)
        est = None if es is None else torch.from_numpy(np.ascontiguousarray(es, np.float32)).cuda()
        if rng:
            b.rng[:2 * n] = (self.rng0 if rng0 is None else rng0).reshape(-1)
        rows = self.rows if rows is None else rows
        ts = self.ts if ts is None else ts
        w = self.seat._w
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        pl = _lib.PolicyLstmPlayer(rows.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), hin.data_ptr(),
                                   cin.data_ptr(), b.h.data_ptr() if write_state else None,
                                   b.c.data_ptr() if write_state else None, ptr(est), b.rng.data_ptr() if rng else None,
                                   ptr(given), b.pairs.data_ptr(), b.move.data_ptr(), b.comm.data_ptr(),
                                   b.log_prob.data_ptr(), b.value.data_ptr(), b.logits.data_ptr())
        rc = L.oc_policy_lstm_ac(ctypes.byref(pl), ts.data_ptr(), self.F, self.C, OT[self.odt], n,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.oc_policy_last_error()
        torch.cuda.synchronize()
        return hin, cin


def _inside(name, got, ref, bound, tag):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("recurrent %s %s: max err %.3g, max bound %.3g, max err/bound %.3f (session max %.3f)"
          % (name, tag, err.max(), bound.max(), ratio, WORST[name]))
    assert (err <= bound).all(), (name, tag, np.argwhere(err > bound)[:5].tolist())


def _check_step(w, rows, ts, h, c, es, got, tag, mutants):
    """got: logits, value, h, c of one launch from (h, c, es).  Every element inside its bound; every planted
    bug of ``mutants`` (True: all of recurrent_ref.MUTANTS) outside it somewhere."""
    em = rr.step(w, rows, ts, h, c, es)
    dh, dc = rr.state_bound(em)
    lb, vb, info = rr.logits_bound(em)
    pairs = (("logits", got.logits, em["logits"], lb), ("value", got.value, em["value"], vb), ("h", got.h, em["h"], dh),
             ("c", got.c, em["c"], dc))
    for name, g, r, bnd in pairs:
        _inside(name, g, r, bnd, tag)
    if mutants:
        for mname in (rr.MUTANTS if mutants is True else mutants):
            mu = rr.step(w, rows, ts, h, c, es, mutate=mname)
            hit = [name for name, g, _, bnd in pairs if (np.abs(np.asarray(g, np.float64) - mu[name]) > bnd).any()]
            print("recurrent mutant %r %s: outside the bound in %s" % (mname, tag, hit))
            assert hit, "the bounds let a planted bug through: " + mname
    return em, info


SHAPES = [(7, 1, "int8"), (29, 2, "int32"), (46, 5, "float32"), (62, 16, "int32")]
SIZES = (1, 31, 32, 33, 64, 100)


@pytest.mark.parametrize("scale", [1, 8], ids=["x1", "x8"])
@pytest.mark.parametrize("F,C,odt", SHAPES, ids=["F%d-C%d-%s" % s for s in SHAPES])
def test_one_step_lies_inside_the_derived_bounds(F, C, odt, scale):
    for n in SIZES:
        case = Case(F, C, odt, n, scale)
        b = Bufs(n, C)
        case.launch(b)
        b.guards_intact()
        tag = "F%d C%d %s n%d x%d" % (F, C, odt, n, scale)
        em, _ = _check_step(case.w, case.rows_np, case.ts_np, case.h_np, case.c_np, case.es_np, b.out(), tag, mutants=n == 100)
        if scale == 8 and n == 100:         # some gates saturate (r is 0 or 1 to float32), some do not
            r = np.stack([em["gi"], em["gf"], em["go"], em["rg"]])
            sat = (r < 2.0 ** -24) | (r > 1 - 2.0 ** -24)
            print("recurrent %s: %.1f %% of the gates saturated" % (tag, 100 * sat.mean()))
            assert sat.any() and not sat.all() and 0.01 < sat.mean() < 0.99


def test_a_starting_env_takes_the_zero_state_whatever_the_old_one_held():
    F, C, odt, n = 29, 2, "int32", 100
    case = Case(F, C, odt, n, 1)
    start = case.es_np > 0
    assert 10 < start.sum() < n - 10
    poisoned_h, poisoned_c = case.h_np.copy(), case.c_np.copy()
    cols = np.flatnonzero(start)
    poisoned_h[:, cols[0::2]], poisoned_c[:, cols[0::2]] = np.nan, np.nan
    poisoned_h[:, cols[1::2]], poisoned_c[:, cols[1::2]] = 1e30, -1e30
    poisoned_h[5, cols[1]], poisoned_c[7, cols[0]] = np.inf, -np.inf
    zero_h, zero_c = np.where(start, np.float32(0), case.h_np), np.where(start, np.float32(0), case.c_np)
    a, z, nul = Bufs(n, C), Bufs(n, C), Bufs(n, C)
    case.launch(a, poisoned_h, poisoned_c)
    case.launch(z, zero_h, zero_c)
    a.guards_intact()
    z.guards_intact()
    for name in ("pairs", "move", "comm", "rng", "log_prob", "value", "logits", "h", "c"):
        assert torch.equal(_bits(getattr(a, name)[:-GUARD]), _bits(getattr(z, name)[:-GUARD])), name
    # the zero state is also what the reference says the step starts from
    _check_step(case.w, case.rows_np, case.ts_np, poisoned_h, poisoned_c, case.es_np, a.out(), "poisoned state", False)
    # episode_start = NULL equals all zeros
    case.launch(a, es=np.zeros(n, np.float32))
    case.launch(nul, es=None)
    for name in ("pairs", "rng", "log_prob", "value", "logits", "h", "c"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(nul, name))), name
    assert not torch.equal(_bits(a.h), _bits(z.h))          # (and the mask did something)


def test_stores_stay_inside_the_batch_and_the_state_may_be_updated_in_place():
    F, C, odt, n = 46, 5, "float32", 33
    case = Case(F, C, odt, n, 1)
    sep, ali, dry = Bufs(n, C), Bufs(n, C), Bufs(n, C)
    hin, cin = case.launch(sep)
    sep.guards_intact()
    # the inputs, and what lies behind them, are as they were
    assert torch.equal(hin[:64 * n].cpu(), torch.from_numpy(case.h_np.reshape(-1))) and torch.isnan(hin[64 * n:]).all()
    assert torch.equal(cin[:64 * n].cpu(), torch.from_numpy(case.c_np.reshape(-1))) and torch.isnan(cin[64 * n:]).all()
    case.launch(ali, alias=True)             # h_out = h_in, c_out = c_in
    ali.guards_intact()
    for name in ("pairs", "move", "comm", "rng", "log_prob", "value", "logits", "h", "c"):
        assert torch.equal(_bits(getattr(sep, name)), _bits(getattr(ali, name))), name
    hin, cin = case.launch(dry, write_state=False)       # h_out = c_out = NULL
    dry.guards_intact(state=False)
    assert torch.equal(hin[:64 * n].cpu(), torch.from_numpy(case.h_np.reshape(-1)))
    for name in ("pairs", "rng", "log_prob", "value", "logits"):
        assert torch.equal(_bits(getattr(sep, name)), _bits(getattr(dry, name))), name
    # greedy: the streams are neither read nor written
    dry = Bufs(n, C)
    case.launch(dry, rng=False)
    dry.guards_intact(rng=False)


def test_an_env_does_not_depend_on_its_batch():
    F, C, odt, n = 62, 16, "int32", 100
    case = Case(F, C, odt, n, 1)
    b = Bufs(n, C)
    case.launch(b)
    full = b.out()
    for e in (0, 31, 32, 99):
        one = Bufs(1, C)
        case.launch(one, h=np.ascontiguousarray(case.h_np[:, e:e + 1]), c=np.ascontiguousarray(case.c_np[:, e:e + 1]),
                    es=case.es_np[e:e + 1], rows=case.rows[:, e:e + 1].contiguous(), ts=case.ts[e:e + 1].contiguous(),
                    rng0=case.rng0[:, e:e + 1].contiguous(), n=1)
        one.guards_intact()
        o = one.out()
        for name in ("logits", "h", "c", "rng"):
            assert np.array_equal(getattr(o, name)[:, 0].view(np.int32), getattr(full, name)[:, e].view(np.int32)), (e, name)
        for name in ("log_prob", "value", "move", "comm"):
            assert np.array_equal(getattr(o, name)[:1].view(np.int32), getattr(full, name)[e:e + 1].view(np.int32)), (e, name)
        assert np.array_equal(o.pairs[0], full.pairs[e])


# ---- the tail -------------------------------------------------------------------------------------
def _lp_from_logits(L, pairs, C):
    """(log_prob, tolerance) in float64 from the kept natural-log logits [4 + C][n] and the pairs.  The kernel
    forms it from the base-2 accumulators the kept logits are the float32 products `out * ln 2` of, so per head
    the kept values carry 2^-22 relative (the product and the rounded constant), twice (L_a and the
    normaliser); behind that the float32 chain policy_ac_ref.log_prob_bound describes: u (|d_a| + max(|g|, 1)
    + |q|) in base 2, rel_S / ln 2 for the sum, 2 u |lp| for the conversion, u |log_prob| for the last add."""
    n = L.shape[1]
    lp, tol, mag = np.zeros(n), np.zeros(n), np.zeros(n)
    for col, (lo, hi) in enumerate(((0, 4), (4, 4 + C))):
        x = L[lo:hi].astype(np.float64)
        count = hi - lo
        m = x.max(axis=0)
        S = np.exp(x - m).sum(axis=0)
        xa = x[pairs[:, col], np.arange(n)]
        term = (xa - m) - np.log(S)
        d_a, g = np.abs(xa - m) / pr.LN2, np.log2(S)
        rel_S = pr._gamma(count - 1) + pr.U_F32 + count * (0.37 * pr.U_F32 + 2.0 ** -126)
        base2 = pr.U_F32 * (d_a + np.maximum(g, 1.0) + d_a + g) + rel_S / (pr.LN2 * (1 - rel_S))
        lp += term
        mag += np.abs(term)
        tol += pr.LN2 * base2 + 2 * pr.U_F32 * np.abs(term) + 2 * 2.0 ** -22 * np.abs(x).max(axis=0)
    return lp, tol + pr.U_F32 * mag


def test_sampled_pairs_follow_the_host_pcg32_and_the_log_prob_its_logits():
    k = rr.sampling_case()
    F, C, n = k["F"], k["C"], k["n"]
    case = Case(F, C, k["odt"], n, 1, pol=k["pol"])
    case.rows_np, case.ts_np = k["rows"], k["ts"]
    case.rows, case.ts = torch.from_numpy(k["rows"]).cuda(), torch.from_numpy(k["ts"]).cuda()
    rng0 = torch.from_numpy(k["rng"]).cuda()
    b = Bufs(n, C)
    case.launch(b, k["h"], k["c"], k["es"], rng0=rng0)
    b.guards_intact()
    o = b.out()
    s_new, draw = pr.pcg32(k["rng"])
    assert np.array_equal(s_new.astype(np.uint32), o.rng.view(np.uint32))          # both streams advanced by one draw
    u = pr.draw_u(draw)
    got = o.logits.astype(np.float64)
    excluded = 0
    for lo, hi, col in ((0, 4, 0), (4, 4 + C, 1)):
        own, margin = pr.ref_sample(got[lo:hi] / pr.LN2, u[col])
        ok = margin >= 1e-5
        excluded += int((~ok).sum())
        assert np.array_equal(o.pairs[ok, col], own[ok]), (col, np.argwhere(o.pairs[ok, col] != own[ok])[:5])
        assert ((o.pairs[:, col] >= 0) & (o.pairs[:, col] < hi - lo)).all()
        assert len(np.unique(o.pairs[:, col])) == hi - lo                         # (every action occurs)
    print("recurrent sampling: %d of %d (env, head) draws excluded" % (excluded, 2 * n))
    assert excluded / (2.0 * n) <= rr.SAMPLING_CAP
    assert np.array_equal(o.move, o.pairs[:, 0]) and np.array_equal(o.comm, o.pairs[:, 1])
    lp, tol = _lp_from_logits(o.logits, o.pairs, C)
    err = np.abs(o.log_prob.astype(np.float64) - lp)
    print("recurrent log_prob from the kept logits: max err %.3g, max err/tol %.3f" % (err.max(), (err / tol).max()))
    assert (err <= tol).all()
    _check_step(k["w"], k["rows"], k["ts"], k["h"], k["c"], k["es"], o, "sampling case", False)

    # greedy: a maximum of its head, the FIRST one where there are several
    case.launch(b, k["h"], k["c"], k["es"], rng=False)
    o = b.out()
    for lo, hi, col in ((0, 4, 0), (4, 4 + C, 1)):
        blk = o.logits[lo:hi]
        assert (blk[o.pairs[:, col], np.arange(n)] == blk.max(axis=0)).all()
        unique = (blk == blk.max(axis=0)).sum(axis=0) == 1
        assert unique.sum() > n // 2 and np.array_equal(o.pairs[unique, col], pr.first_argmax(blk)[unique])
    tie = rr.make_module(F, C, 3, 1)
    with torch.no_grad():
        for t in (tie.w2, tie.wv):
            t.zero_()
        bias = [1.0, 1.0, 0.0, 1.0] + [0.5] * C
        bias[4] = -0.25                  # a lower first comm logit: the first of the tied maxima is comm 1
        tie.b2.copy_(torch.tensor(bias).view(-1, 1))
    tcase = Case(F, C, k["odt"], 97, 1, pol=tie)
    tb = Bufs(97, C)
    tcase.launch(tb, rng=False)
    o = tb.out()
    assert (o.pairs[:, 0] == 0).all() and (o.pairs[:, 1] == 1).all()
    assert (o.logits[0] == o.logits[1]).all() and (o.logits[5:] == o.logits[5]).all()


def test_score_returns_the_recorded_bits_and_writes_no_seat_state():
    from gym_comm_amd.vec_env import FusedRecurrentPartner
    F, C, odt, n = 29, 2, "float32", 97
    case = Case(F, C, odt, n, 4)
    seat = FusedRecurrentPartner(case.pol, sample=True, seed=8, keep_logits=True)
    obs = SimpleNamespace(rows=case.rows, timestep=case.ts)
    act = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    seat.act_into(obs, act[0], act[1])                                 # a first step: every env starts
    seat.update(torch.zeros(n, dtype=torch.float64, device="cuda"), (torch.arange(n, device="cuda") % 3 == 0).to(torch.int32))
    assert seat.h.abs().max() > 0 and 0 < int(seat.episode_start.sum().item()) < n
    h0, c0, es0 = seat.h.clone(), seat.c.clone(), seat.episode_start.clone()
    seat.act_into(obs, act[0], act[1])                                 # the recorded step, from (h0, c0, es0)
    pairs = act.T.contiguous()
    held = [seat._rng, seat.episode_start, seat.log_prob, seat.value, seat.logits, seat.h, seat.c]
    before = [(t.data_ptr(), t.clone()) for t in held]
    lp, val = seat.score(obs, (h0, c0), es0, pairs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lp), _bits(seat.log_prob)) and torch.equal(_bits(val), _bits(seat.value))
    for t, (ptr, was) in zip([seat._rng, seat.episode_start, seat.log_prob, seat.value, seat.logits, seat.h, seat.c], before):
        assert t.data_ptr() == ptr and torch.equal(_bits(t), _bits(was))
    assert not torch.equal(h0, seat.h)                                 # (the recorded step moved the state)
    # a batch of another size, scored by a seat that has never acted: nothing is allocated for it
    fresh = FusedRecurrentPartner(case.pol, sample=True, seed=9)
    k = 33
    sub = SimpleNamespace(rows=case.rows[:, :k].contiguous(), timestep=case.ts[:k].contiguous())
    lp2, val2 = fresh.score(sub, (h0[:, :k].contiguous(), c0[:, :k].contiguous()), es0[:k].contiguous(), pairs[:k].contiguous())
    assert torch.equal(_bits(lp2), _bits(lp[:k])) and torch.equal(_bits(val2), _bits(val[:k]))
    assert fresh.h is None and fresh._rng is None and fresh.log_prob is None
    # an index outside its head's range: -inf for that env only
    bad = pairs.clone()
    bad[0, 0], bad[n // 2, 1], bad[n - 1, 1] = 4, C, -1
    lp3, val3 = seat.score(obs, (h0, c0), es0, bad)
    hit = [0, n // 2, n - 1]
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[hit] = False
    assert torch.isneginf(lp3[hit]).all() and torch.equal(_bits(lp3[rest]), _bits(lp[rest])) and torch.equal(_bits(val3), _bits(val))
    # the raw launch echoes the index it was given, in range or not; the state it writes is the recorded one
    b = Bufs(n, C)
    case.launch(b, h0.cpu().numpy(), c0.cpu().numpy(), es0.cpu().numpy(), rng=False, given=bad)
    b.guards_intact(rng=False, finite=False)
    assert torch.equal(b.pairs[:2 * n].view(n, 2), bad) and torch.equal(b.move[:n], bad[:, 0]) and torch.equal(b.comm[:n], bad[:, 1])
    assert torch.equal(_bits(b.log_prob[:n]), _bits(lp3)) and torch.equal(_bits(b.h[:64 * n].view(64, n)), _bits(seat.h))
    with pytest.raises(ValueError):
        seat.score(obs, (h0.T.contiguous(), c0), es0, pairs)
    with pytest.raises(TypeError):
        from gym_comm_amd.vec_env import MLPActorCritic
        FusedRecurrentPartner(MLPActorCritic(3, C))


# ---- the seat in the env ----------------------------------------------------------------------------
SC, ST, SN, TMAX = 2, 60, 64, 25


def _seat(graph):
    from gym_comm_amd.vec_env import FusedRecurrentPartner, LSTMActorCritic, OvercookedVecEnv, RolloutSink
    arg = SimpleNamespace(level="open-divider_tomato", num_agents=2, max_num_timesteps=TMAX, ego_config={},
                          partner_config={}, num_communication=SC, communication_on=True, ego_led=False, fow_radius=2)
    venv = OvercookedVecEnv(arg, SN, seed=5, obs_dtype=torch.float32, use_graph=graph)
    F = 22 + venv._b.S + 2 * SC
    pol = LSTMActorCritic(venv._b.S, SC, seed=31)
    with torch.no_grad():
        for t in pol.parameters():
            t.mul_(4)
    pol = pol.cuda()
    sink = RolloutSink(ST, SN, F, obs_dtype=torch.float32, fused=True)
    venv.partner = seat = FusedRecurrentPartner(pol, sample=True, seed=12, sink=sink, keep_logits=True)
    venv.reset_tensors()
    g = torch.Generator().manual_seed(9)
    ego = torch.stack([torch.randint(0, 4, (ST, SN), generator=g), torch.randint(0, SC, (ST, SN), generator=g)], dim=2)
    return SimpleNamespace(venv=venv, pol=pol, sink=sink, seat=seat, ego=ego.to(torch.int32).cuda(), F=F)


def _sink_tensors(s):
    return [s.obs, s.timestep, s.actions, s.log_probs, s.values, s.rewards, s.episode_starts, s.dones, s.pos, s.last, s.count]


def test_the_seat_in_the_env_eager_and_captured_step_by_step():
    from gym_comm_amd import _lib
    e = _seat(False)
    assert e.seat.graph_safe
    pre_h, pre_c, logits = [], [], []
    for k in range(ST):
        e.seat._buffers(SN)
        pre_h.append(e.seat.h.clone())
        pre_c.append(e.seat.c.clone())
        e.venv.step_tensors(e.ego[k])
        logits.append(e.seat.logits.clone())
    pre_h.append(e.seat.h.clone())
    pre_c.append(e.seat.c.clone())
    s = e.sink
    assert s.steps() == ST and s.full()
    es = s.episode_starts.cpu().numpy()
    assert (es[0] == 1).all() and (es[1:].sum(axis=0) >= 2).all() and es[1:].mean() < 0.2      # every env reset, twice
    w = rr.weights(e.pol)
    worst = {"logits": 0.0, "value": 0.0}
    # mutants here too: the one that misses the mask where most envs start, four others at a step where none
    # does (a starting env's timestep is 0 and its old h is not read: there they would change nothing)
    kmut = 1 + int(es[1:].sum(axis=1).argmax())
    quiet = [k for k in range(2, ST) if es[k].sum() == 0]
    assert es[kmut].sum() > 0 and quiet
    planted = {kmut: ["f applied to c_prev unmasked"],
               quiet[-1]: ["g/o swapped", "timestep column dropped", "b dropped", "tanh(c) replaced by c"]}
    for k in range(ST):
        rows, ts = s.obs[k].cpu().numpy(), s.timestep[k].cpu().numpy()
        got = SimpleNamespace(logits=logits[k].cpu().numpy(), value=s.values[k].cpu().numpy(), h=pre_h[k + 1].cpu().numpy(),
                              c=pre_c[k + 1].cpu().numpy())
        h, c = pre_h[k].cpu().numpy(), pre_c[k].cpu().numpy()
        _check_step(w, rows, ts, h, c, es[k], got, "env step %d" % k, mutants=planted.get(k, False))
        ex = rr.step(w, rows, ts, h, c, es[k], emulate=False)
        worst["logits"] = max(worst["logits"], float(np.abs(got.logits - ex["logits"]).max()))
        worst["value"] = max(worst["value"], float(np.abs(got.value - ex["value"]).max()))
        # the recorded log-probability is that of the recorded action under the kept logits
        lp, tol = _lp_from_logits(got.logits, s.actions[k].T.cpu().numpy(), SC)
        assert (np.abs(s.log_probs[k].cpu().numpy() - lp) <= tol).all(), k
    print("recurrent seat against the plain float32 module over %d steps: logits %.3g, value %.3g"
          % (ST, worst["logits"], worst["value"]))
    assert worst["logits"] <= 2 * PLAIN_LOGITS and worst["value"] <= 2 * PLAIN_VALUE

    # envs that reset show a zeroed input state: the recorded step is, bit for bit, a launch that is handed
    # zeros in those envs' columns and no episode_start at all
    L = _lib.load(lib="policy")
    shown = 0
    for k in range(1, ST):
        start = es[k] > 0
        if not start.any() or shown == 3:
            continue
        shown += 1
        assert (pre_h[k][:, torch.from_numpy(start).cuda()].abs().max(dim=0).values > 0).all()      # there was a state to forget
        gone = torch.from_numpy(start).cuda().unsqueeze(0)
        h0, c0 = torch.where(gone, 0.0, pre_h[k]).contiguous(), torch.where(gone, 0.0, pre_c[k]).contiguous()
        h1, c1 = torch.empty_like(h0), torch.empty_like(c0)
        given = s.actions[k].T.contiguous()
        lp, val = torch.empty(SN, device="cuda"), torch.empty(SN, device="cuda")
        sw = e.seat._w
        pl = _lib.PolicyLstmPlayer(s.obs[k].data_ptr(), sw[0].data_ptr(), sw[1].data_ptr(), sw[2].data_ptr(), h0.data_ptr(),
                                   c0.data_ptr(), h1.data_ptr(), c1.data_ptr(), None, None, given.data_ptr(), None, None, None,
                                   lp.data_ptr(), val.data_ptr(), None)
        assert L.oc_policy_lstm_ac(ctypes.byref(pl), s.timestep[k].data_ptr(), e.F, SC, OT["float32"], SN,
                                   torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(h1), _bits(pre_h[k + 1])) and torch.equal(_bits(c1), _bits(pre_c[k + 1]))
        assert torch.equal(_bits(lp), _bits(s.log_probs[k])) and torch.equal(_bits(val), _bits(s.values[k]))
    assert shown >= 2          # (the time limit ends every episode at steps 25 and 50)

    # returns and advantages come from the seat's last value and episode_start, as for the other recording seats
    adv, ret = e.seat.finish_rollout()
    assert tuple(adv.shape) == (ST, SN) and torch.isfinite(adv).all() and torch.isfinite(ret).all()

    # the same run with the partner, the step and the update captured (use_graph=True)
    g = _seat(True)
    for k in range(ST):
        g.venv.step_tensors(g.ego[k])
    torch.cuda.synchronize()
    for a, b in zip(_sink_tensors(g.sink), _sink_tensors(s)):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(g.seat.get_state(SN), e.seat.get_state(SN)):
        if isinstance(a, torch.Tensor):
            assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(g.seat.h), _bits(e.seat.h)) and torch.equal(_bits(g.seat.c), _bits(e.seat.c))
    assert torch.equal(g.seat._rng, e.seat._rng)
    assert torch.equal(g.venv._b._arena, e.venv._b._arena) and torch.equal(g.venv._act, e.venv._act)

    # reset(): every env starts again, and get_state / set_state carry h and c
    st = e.seat.get_state(SN)
    e.venv.step_tensors(e.ego[0])
    assert not torch.equal(e.seat.h, st[5])
    e.seat.set_state(st)
    assert torch.equal(_bits(e.seat.h), _bits(st[5])) and torch.equal(_bits(e.seat.c), _bits(st[6])) and torch.equal(e.seat._rng, st[0])
    e.venv.reset_tensors()
    assert (e.seat.episode_start == 1).all()
