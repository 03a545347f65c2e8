"""A float64 restatement of the recurrent seat (include/oc_policy.h, last section: oc_policy_lstm_ac) for
the tests -- not a test module.  Like tests/policy_ref.py, on which it builds, it is written from the
module's plain weights (vec_env.LSTMActorCritic: wx [256][F], wt [256], b [256], wh [256][64], w2 [4 + C][64],
b2 [4 + C], wv [64], bv [1]) and the header's text, never from the packed images.

    step(w, rows, ts, h, c, es, emulate=False)   the exact module in float64
    step(w, rows, ts, h, c, es, emulate=True)    the same with exactly the roundings the header names, and
                                                 nothing else; ``mutate`` plants a bug (the tests' mutants)
    state_bound(f) / logits_bound(f, ...)        how far the kernel's h, c / logits, value may lie from the
                                                 emulated ones (f = the dict an emulated step returns)

State is feature-major float [64][n] as the kernel keeps it; logits natural-log [4 + C][n].
"""
import numpy as np

import policy_ref as pr

H = 64
U = pr.U_F32                                  # 2^-23: one fp32 ulp, charged for every fp32 operation
LOG2E32 = pr.LOG2E32
K_TANH = float(np.float32(2) * LOG2E32)       # the float the kernel multiplies c by
TINY = 2.0 ** -126                            # a result below the normal range may be flushed
MUTANTS = ("g/o swapped", "f applied to c_prev unmasked", "h fed unrounded", "timestep column dropped", "b dropped",
           "tanh(c) replaced by c")


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def weights(pol):
    """(wx, wt, b, wh, w2, b2, wv, bv) of a module as float64 arrays, the vectors flat."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    return (f(pol.wx), f(pol.wt).reshape(-1), f(pol.b).reshape(-1), f(pol.wh), f(pol.w2), f(pol.b2).reshape(-1),
            f(pol.wv).reshape(-1), f(pol.bv).reshape(-1))


def fold_gates(wx, wt, b, wh):
    """The fp16 values the gate product multiplies by, float64 [256][F + 2 + 64]: -log2(e) [Wx | wt | b | Wh] for
    the rows of i, f, o and 2 log2(e) [...] for g's (rows 128..191), the product in fp32, rounded once."""
    aug = np.concatenate([np.asarray(wx, np.float32), np.asarray(wt, np.float32).reshape(-1, 1),
                          np.asarray(b, np.float32).reshape(-1, 1), np.asarray(wh, np.float32)], axis=1)
    scale = np.full((4 * H, 1), -LOG2E32, np.float32)
    scale[2 * H:3 * H] = np.float32(2) * LOG2E32
    return _f16((scale * aug).astype(np.float32))


def fold_head(w2, wv, b2, bv):
    """(log2(e) [W2; wv] in fp16, log2(e) [b2; bv] in fp32) as float64: [5 + C][64], [5 + C]; the value last."""
    w = np.concatenate([np.asarray(w2, np.float32), np.asarray(wv, np.float32).reshape(1, -1)])
    bias = np.concatenate([np.asarray(b2, np.float32).reshape(-1), np.asarray(bv, np.float32).reshape(-1)])
    return _f16((LOG2E32 * w).astype(np.float32)), (LOG2E32 * bias).astype(np.float32).astype(np.float64)


def _r(a):
    with np.errstate(over="ignore"):
        return 1.0 / (np.exp2(a) + 1.0)


def step(w, rows, ts, h, c, es=None, emulate=True, mutate=None):
    """One step for n envs.  rows [F][n] (any row type), ts [n], h / c float [64][n] (the STORED float32
    state), es [n] or None.  Returns a dict: logits [4 + C][n] (natural log), value [n], h, c [64][n] and,
    emulated, the intermediates the bounds need."""
    if mutate is not None and mutate not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutate,))
    wx, wt, b, wh, w2, b2, wv, bv = (np.asarray(t, np.float64) for t in w)
    n = np.asarray(rows).shape[1]
    start = np.zeros(n, bool) if es is None else np.asarray(es) > 0
    h_prev = np.asarray(h, np.float32).astype(np.float64)
    c_prev = np.asarray(c, np.float32).astype(np.float64)
    h_in, c_in = np.where(start, 0.0, h_prev), np.where(start, 0.0, c_prev)       # a select: NaN does not survive
    if not emulate:
        x = np.asarray(rows).astype(np.float64)
        z = wx @ x + wt.reshape(-1, 1) * np.asarray(ts, np.float64).reshape(1, -1) + b.reshape(-1, 1) + wh @ h_in
        zi, zf, zg, zo = z.reshape(4, H, n)
        with np.errstate(over="ignore"):
            sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
            cn = sig(zf) * c_in + sig(zi) * np.tanh(zg)
            hn = sig(zo) * np.tanh(cn)
        return dict(logits=w2 @ hn + b2.reshape(-1, 1), value=wv @ hn + bv[0], h=hn, c=cn)
    A = fold_gates(wx, wt, b, wh)
    X = pr.features(rows, ts)                                                     # [F + 2][n], fp16 values
    F = X.shape[0] - 2
    if mutate == "timestep column dropped":
        X[F] = 0.0
    if mutate == "b dropped":
        X[F + 1] = 0.0
    B = np.concatenate([X, h_in if mutate == "h fed unrounded" else _f16(h_in)])  # [F + 2 + 64][n]
    a = A @ B                                                                     # fp16 x fp16 products: exact
    ai, af, ag, ao = a.reshape(4, H, n)
    if mutate == "g/o swapped":
        ag, ao = ao, ag
    gi, gf, go = _r(ai), _r(af), _r(ao)
    rg = _r(ag)
    gg = 1.0 - 2.0 * rg
    c_used = c_prev if mutate == "f applied to c_prev unmasked" else c_in
    with np.errstate(invalid="ignore"):
        cn = gf * c_used + gi * gg
    rc = _r(K_TANH * cn)
    th = cn if mutate == "tanh(c) replaced by c" else 1.0 - 2.0 * rc
    hn = go * th
    Wh16, bias = fold_head(w2, wv, b2, bv)
    h16 = _f16(hn)
    L2 = Wh16 @ h16 + bias.reshape(-1, 1)                                         # base 2; the value last
    return dict(logits=L2[:-1] * pr.LN2, value=L2[-1] * pr.LN2, h=hn, c=cn, A=A, B=B, a=a, gi=gi, gf=gf, go=go, rg=rg,
                gg=gg, c_in=c_in, rc=rc, th=th, Wh16=Wh16, bias=bias, h16=h16, L2=L2, kx=(F + 2 + 15) // 16)


def _dr(r, da):
    """How far the kernel's r = v_rcp_f32(v_exp_f32(a') + 1) may lie from 1 / (2^a + 1) when |a' - a| <= da:
    the function moves by at most ln 2 max r (1 - r) da (max over the interval <= r (1 - r) 2^da, <= 1/4),
    the three instructions add EPS_R relative (policy_ref), a result below 2^-126 may be flushed."""
    rr = np.minimum(0.25, r * (1.0 - r) * np.exp2(np.minimum(da, 64.0)))
    return pr.LN2 * rr * da * (1 + pr.EPS_R) + pr.EPS_R * r + TINY


def state_bound(f):
    """(dh, dc), [64][n] each: per-element bounds on |kernel - emulated| for the stored h and c.

    After emulation the kernel differs in this only:
    1. fp32 accumulation inside the MFMAs: a gate row sums K = 16 ksteps + 64 + 1 exact products (the x
       k-steps, the 64 units of h, the start value), so |a' - a| <= da = gamma(K) sum |A_k B_k|.
    2. each r through ``_dr``.  g = 1 - 2 r: the doubling is exact, the subtraction rounds once.
    3. the cell in float32, operation by operation, u = 2^-23 each: t1 = f c_in, t2 = i g, c = t1 + t2;
       ac = K_TANH c; r_c through ``_dr`` with dac = K_TANH dc + u |ac|; tanh = 1 - 2 r_c; h = o tanh.
       Each operation may also flush a result below the normal range: 2^-126 each.
    First-order terms and their products are all kept (no 'higher order terms dropped')."""
    da = pr._gamma(16 * f["kx"] + H + 1) * (np.abs(f["A"]) @ np.abs(f["B"]))
    dai, daf, dag, dao = da.reshape(4, H, -1)
    gi, gf, go, gg = f["gi"], f["gf"], f["go"], f["gg"]
    di, df, do = _dr(gi, dai), _dr(gf, daf), _dr(go, dao)
    dg = 2 * _dr(f["rg"], dag)
    dg = dg + U * (np.abs(gg) + dg) + TINY
    cin = np.abs(f["c_in"])
    t1, t2 = gf * cin, np.abs(gi * gg)
    e1 = df * cin + U * (gf + df) * cin + TINY
    e2 = di * np.abs(gg) + dg * gi + di * dg + U * (gi + di) * (np.abs(gg) + dg) + TINY
    dc = e1 + e2 + U * (t1 + t2 + e1 + e2) + TINY
    ac = K_TANH * np.abs(f["c"])
    dac = K_TANH * dc + U * (ac + K_TANH * dc) + TINY
    dth = 2 * _dr(f["rc"], dac)
    dth = dth + U * (np.abs(f["th"]) + dth) + TINY
    th = np.abs(f["th"])
    dh = do * th + dth * go + do * dth + U * (go + do) * (th + dth) + TINY
    return dh, dc


def logits_bound(f):
    """(bound on the logits [4 + C][n], bound on the value [n], info): |kernel - emulated|, natural log.

    The head product takes fp16(h).  The kernel's h lies within dh (``state_bound``) of the emulated one, so
    its rounding lands on the same fp16 value unless the emulated h lies within dh of a rounding midpoint:
    only such units are charged, one fp16 ulp of h (the larger neighbour gap) times |W_oj| each.  The product
    itself: 64 terms and the start value, gamma(64 + 1 + 1) as policy_ref charges its second product.  The
    sum is in base 2; ln 2 converts it and the kernel's ``out * K_LN2`` adds 2^-22 |logit| (policy_ref)."""
    dh, _ = state_bound(f)
    h, h16 = f["h"], f["h16"]
    q = h16.astype(np.float16)
    lo = np.nextafter(q, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(q, np.float16(np.inf)).astype(np.float64)
    dist = np.minimum(np.abs(h - 0.5 * (lo + h16)), np.abs(h - 0.5 * (h16 + hi)))
    ulp = np.maximum(h16 - lo, hi - h16)
    flip = (dist <= dh).astype(np.float64)
    Wa = np.abs(f["Wh16"])
    b2 = Wa @ (flip * ulp) + pr._gamma(H + 2) * (np.abs(f["bias"]).reshape(-1, 1) + Wa @ (np.abs(h16) + ulp))
    nat = pr.LN2 * b2 + 2.0 ** -22 * np.abs(f["L2"] * pr.LN2)
    return nat[:-1], nat[-1], dict(flipped=flip, dh=dh)


def make_module(F, C, seed, scale):
    """``LSTMActorCritic(seed)`` (CPU) with its input weights re-drawn for F features (same init rule) and
    every weight scaled by `scale`."""
    import torch
    from gym_comm_amd.vec_env import LSTMActorCritic
    pol = LSTMActorCritic(3, C, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        pol.wx = torch.nn.Parameter((torch.rand((4 * H, F), generator=g) * 2 - 1) / float(np.sqrt(F)))
        for t in pol.parameters():
            t.mul_(scale)
    return pol


def make_rows(F, n, odt, seed):
    """Observation rows [F][n]: small values, one element in fifty from the type's whole range (so that
    most envs see small features only and their bounds are tight), both ends present."""
    rng = np.random.default_rng(seed)
    if odt == "float32":
        small, big, lo, hi = rng.uniform(-2, 2, (F, n)), rng.uniform(-2048, 2048, (F, n)), -2047.7, 2047.3
    else:
        lo, hi = (-128, 127) if odt == "int8" else (-2048, 2048)
        small, big = rng.integers(-2, 3, (F, n)), rng.integers(lo, hi + 1, (F, n))
    x = np.where(rng.random((F, n)) < 0.02, big, small)
    x.flat[0] = lo
    x.flat[-1] = hi
    return x.astype({"int32": np.int32, "int8": np.int8, "float32": np.float32}[odt])


def make_state(n, seed):
    """(h, c, episode_start): state uniform in +-1, float32 [64][n]; about a third of the envs start."""
    rng = np.random.default_rng(seed + 31)
    es = (rng.random(n) < 0.35).astype(np.float32)
    return (rng.uniform(-1, 1, (H, n)).astype(np.float32), rng.uniform(-1, 1, (H, n)).astype(np.float32), es)


# ---- the sampling case of tests/test_recurrent_seat_gpu.py, shared with the CPU test of its seed ------
SAMPLING_CAP = 0.005          # the share of (env, head) draws that may be excluded for a margin below 1e-5


def sampling_case():
    """Module, inputs and the seat's initial stream states (uint32 bit patterns, [2][n]) of the case."""
    from gym_comm_amd.batched import pcg32_seed_states
    F, C, n, seed = 29, 5, 1000, 77
    pol = make_module(F, C, 21, 2)
    h, c, es = make_state(n, 8)
    return dict(F=F, C=C, n=n, odt="int8", seed=seed, pol=pol, w=weights(pol), rows=make_rows(F, n, "int8", 15),
                ts=np.random.default_rng(6).integers(0, 334, n) / 333.0, h=h, c=c, es=es,
                rng=pcg32_seed_states(seed, (2, n), "cpu").numpy())
