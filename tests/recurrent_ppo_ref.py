"""A float64 restatement of the recurrent PPO update (include/oc_policy.h, last section: oc_policy_rppo_update /
oc_policy_rppo_grad) for the tests -- not a test module.  It builds on tests/recurrent_ref.py (the step) and
tests/ppo_ref.py (the loss's heads, the clip, Adam), and is written from the module's plain weights and the
header's equations, never from the packed images.

    loss_and_grad(case, hp, emulate, mutate)   the loss terms, the ten statistics' raw values and the UNCLIPPED
                                               gradient of the eight tensors over whole sequences
    clip / adam / adam_bound / HP              ppo_ref's
    make_case(T, n, envs, F, C, odt, seed...)  the inputs the CPU and the GPU tests share
    MUTANTS                                    bugs ``mutate`` plants
    gpu_cases() / edge_cases()                 the cases a-c / d-g of the GPU tests

``emulate=True`` runs ``recurrent_ref.step(emulate=True)`` step by step -- each step from the previous one's
state, stored as float32 -- and takes the derivatives where the header says the kernel does: at the network
the images represent (the folded fp16 weights divided back by their folds, fp16 features and fp16(h) in the
products), sigma' = r (1 - r) and tanh' = 4 r (1 - r) from the unrounded r, the roundings not differentiated.
``emulate=False`` is the exact module in float64.

Tolerances.  A derived bound through T steps of backpropagation is out of reach here; TOL_G and TOL_S are
4 x the largest |kernel - loss_and_grad(emulate=True)| MEASURED on an MI355X over the cases a-c of
tests/test_recurrent_ppo_gpu.py (figures below; measured, not a bound), and are kept honest by
TOL_G <= MUT_MIN / 20: every planted bug moves some tensor at least twenty times further.  ``edge_cases`` adds
the shapes a full-size minibatch reaches; its 52-step case d has tolerances of its own, TOL_G_LONG / TOL_S_LONG,
made the same way from d's own figures (``tolerances(name)`` picks the pair).
"""
import numpy as np

import policy_ref as pr
import ppo_ref as pp
import recurrent_ref as rr

H = rr.H
NAMES = ("wx", "wt", "b", "wh", "w2", "b2", "wv", "bv")
STATS = pp.STATS
HP, clip, adam, adam_bound = pp.HP, pp.clip, pp.adam, pp.adam_bound
LN2_32 = float(np.float32(0.6931471805599453))          # the float the images' inverse folds use
MUTANTS = ("recurrent dh dropped", "dc f carry dropped", "not cut at starts", "gWh against h_t", "c_in unmasked in dz_f",
           "wrong g derivative", "last step's head term dropped", "divisor T n")

# ---- measured on an MI355X, 2026-10-20, tests/test_recurrent_ppo_gpu.py cases a, b, c (max_groups 0 and 1) ----
# grad: per tensor max |kernel - reference| / max |reference| (``rel_diff``), the largest over the eight tensors
# of a case; stats: the largest |kernel - reference| / max(1, |reference|) (``stats_diff``) over the ten.  The
# largest gradient figure is case b's w2: the kernel's float32 h and the reference's float64 h round to
# different fp16 neighbours in a few elements, and the head's gradient takes fp16(h) as its operand.
MEASURED = dict(grad=dict(a=9.06e-07, b=6.78e-05, c=2.74e-05, c_one_group=2.74e-05),
                stats=dict(a=1.56e-07, b=2.77e-07, c=5.36e-07))
TOL_G = 2.8e-4        # 4 x 6.78e-05, rounded up
TOL_S = 2.2e-6        # 4 x 5.36e-07, rounded up
# the smallest relative move of any tensor's gradient under any mutant, over the cases in which the mutant
# applies (tests/test_recurrent_ppo_cpu.py recomputes it and prints it)
MUT_MIN = 0.0399

# ---- measured on an MI355X, 2026-10-21, the cases of ``edge_cases`` (tests/test_recurrent_ppo_gpu.py) ----
# the same two figures.  e, e48, f, g are short cases with a-c's arithmetic and keep TOL_G / TOL_S; their figures
# are recorded only (each the larger of max_groups 0 and 1).  d runs 52 steps: d_0, d_1, d_7 are max_groups 0 (256
# workgroups, 2 rounds), 1 (260 rounds) and 7 (38 rounds).
MEASURED_EDGE = dict(grad=dict(d_0=1.796e-05, d_1=1.784e-05, d_7=1.792e-05, e=5.38e-06, e48=1.32e-06, f=2.16e-06,
                               g=2.47e-06),
                     stats=dict(d_0=6.45e-08, d_1=7.20e-08, d_7=6.45e-08, e=5.57e-07, e48=2.01e-07, f=5.82e-08,
                                g=1.38e-06))
MEASURED["grad"].update(MEASURED_EDGE["grad"])
MEASURED["stats"].update(MEASURED_EDGE["stats"])
# the long case's tolerances: 4 x the largest figure of d, rounded up -- the margin TOL_G has, for the same reason
# (which fp16 neighbour an h rounds to differs between the kernel's float32 and the reference's float64) -- and
# kept honest by TOL_G_LONG <= (the smallest mutant move of d) / 20 = 0.0515 / 20 (tests/test_recurrent_ppo_cpu.py)
TOL_G_LONG = 7.2e-5   # 4 x 1.796e-05, rounded up
TOL_S_LONG = 2.9e-7   # 4 x 7.20e-08, rounded up


def test_hp(max_grad_norm=1e9):
    """The gradient tests' hyper-parameters: an entropy term that matters; the norm clip off unless asked for."""
    return HP(ent_coef=0.01, max_grad_norm=max_grad_norm, lr=3e-3)


# ---- the forward over whole sequences -------------------------------------------------------------------------
def _exact_step(w, rows, ts, h, c, es):
    wx, wt, b, wh, w2, b2, wv, bv = (np.asarray(t, np.float64) for t in w)
    n = rows.shape[1]
    start = np.asarray(es) > 0
    h_in, c_in = np.where(start, 0.0, h), np.where(start, 0.0, c)
    x = np.concatenate([rows.astype(np.float64), np.asarray(ts, np.float64).reshape(1, -1), np.ones((1, n))])
    z = np.concatenate([wx, wt.reshape(-1, 1), b.reshape(-1, 1)], axis=1) @ x + wh @ h_in
    zi, zf, zg, zo = z.reshape(4, H, n)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    i, f, g, o = sig(zi), sig(zf), np.tanh(zg), sig(zo)
    cn = f * c_in + i * g
    th = np.tanh(cn)
    hn = o * th
    Wg = np.concatenate([wx, wt.reshape(-1, 1), b.reshape(-1, 1), wh], axis=1)
    Whd = np.concatenate([w2, wv.reshape(1, -1)])
    out = Whd @ hn + np.concatenate([b2, bv]).reshape(-1, 1)
    return dict(i=i, f=f, g=g, o=o, di=i * (1 - i), df=f * (1 - f), dg=1 - g * g, do=o * (1 - o), th=th, dth=1 - th * th,
                c_in=c_in, c_prev=np.asarray(c, np.float64), opx=x, oph=h_in, h=hn, c=cn, hhead=hn, logits=out[:-1],
                value=out[-1], Wg=Wg, Whd=Whd, start=start)


def _emulated_step(w, rows, ts, h, c, es):
    f = rr.step(w, rows, ts, h, c, es, emulate=True)
    F = rows.shape[0]
    unfold = np.full((4 * H, 1), -LN2_32)
    unfold[2 * H:3 * H] = 0.5 * LN2_32
    i, ff, o, rg, rc = f["gi"], f["gf"], f["go"], f["rg"], f["rc"]
    return dict(i=i, f=ff, g=f["gg"], o=o, di=i * (1 - i), df=ff * (1 - ff), dg=4 * rg * (1 - rg), do=o * (1 - o),
                th=f["th"], dth=4 * rc * (1 - rc), c_in=f["c_in"], c_prev=np.asarray(c, np.float32).astype(np.float64),
                opx=f["B"][:F + 2], oph=f["B"][F + 2:], h=f["h"], c=f["c"], hhead=f["h16"], logits=f["logits"],
                value=f["value"], Wg=f["A"] * unfold, Whd=f["Wh16"] * LN2_32, start=np.asarray(es) > 0)


def forward(case, emulate=True):
    """The T steps of the minibatch's E sequences from (h0, c0): a list of per-step dicts."""
    envs = np.asarray(case["envs"], np.int64)
    h, c = case["h0"][:, envs], case["c0"][:, envs]
    steps = []
    for t in range(case["obs"].shape[0]):
        rows, ts, es = case["obs"][t][:, envs], case["ts"][t][envs], case["es"][t][envs]
        s = (_emulated_step if emulate else _exact_step)(case["w"], rows, ts, h, c, es)
        if emulate:
            h, c = s["h"].astype(np.float32), s["c"].astype(np.float32)      # the state is stored as float32
        else:
            h, c = s["h"], s["c"]
        steps.append(s)
    return steps


def loss_and_grad(case, hp, emulate=True, mutate=None, steps=None):
    """The header's loss over the B = E T samples of ``case`` and its gradient through time, in float64.
    Returns (grads {name: array shaped as the module's parameter}, stats {name: value}, intermediates).
    ``steps``: ``forward(case, emulate)`` made earlier (the intermediates' "steps"; it is only read): no mutant
    touches the forward, and at T = 52 the forward is nearly all of the time."""
    if mutate is not None and mutate not in MUTANTS:
        raise ValueError("unknown mutant %r" % (mutate,))
    envs = np.asarray(case["envs"], np.int64)
    T, F, n = case["obs"].shape
    E = envs.shape[0]
    B = E * T
    steps = forward(case, emulate) if steps is None else steps
    gather = lambda a: np.asarray(a, np.float64)[:, envs].reshape(-1)  # noqa: E731  (sample i = t E + e)
    adv, ret, old = gather(case["adv"]), gather(case["ret"]), gather(case["old_lp"])
    logits = np.concatenate([s["logits"] for s in steps], axis=1)           # [4 + C][B]
    value = np.concatenate([s["value"] for s in steps])
    actions = np.concatenate([case["actions"][t][:, envs].T for t in range(T)])      # [B][2]
    mean, std = adv.mean(), adv.std(ddof=1)
    ahat = (adv - mean) / (std + 1e-8)
    heads = pp._heads(logits, actions)
    good = heads[0][6] & heads[1][6]
    k1 = good.astype(np.float64)
    lp = np.zeros(B)
    for lo, hi, p, ls, Hh, hot, ok in heads:
        lp += (ls * hot).sum(axis=0)
    lp0 = np.where(good, lp, 0.0)
    ratio = np.where(good, np.exp(lp0 - old), 0.0)
    t1 = ahat * ratio
    t2 = ahat * np.clip(ratio, 1 - hp.clip, 1 + hp.clip)
    inside = (ratio >= 1 - hp.clip) & (ratio <= 1 + hp.clip)
    glp = np.where((t1 <= t2) | inside, -t1, 0.0)
    D = np.zeros((logits.shape[0] + 1, B))                                  # d (B loss) / d [logits; value]
    H_all = np.zeros(B)
    for lo, hi, p, ls, Hh, hot, ok in heads:
        D[lo:hi] = glp * (hot - p) + hp.ent * p * (ls + Hh)
        H_all += Hh
    D[-1] = 2.0 * hp.vf * (value - ret)
    D *= k1

    # ---- backwards through time (the header's equations) ----
    C = logits.shape[0] - 4
    gWg, gWhd, gbh = np.zeros((4 * H, F + 2 + H)), np.zeros((5 + C, H)), np.zeros(5 + C)
    dh_next, dc_next = np.zeros((H, E)), np.zeros((H, E))
    for t in range(T - 1, -1, -1):
        s = steps[t]
        Dt = D[:, t * E:(t + 1) * E]
        head = s["Whd"].T @ Dt
        if mutate == "last step's head term dropped" and t == T - 1:
            head = 0.0 * head
        dh = head + (0.0 if mutate == "recurrent dh dropped" else dh_next)
        do = dh * s["th"]
        dc = (0.0 if mutate == "dc f carry dropped" else dc_next) + dh * s["o"] * s["dth"]
        dz = np.concatenate([dc * s["g"] * s["di"],
                             dc * (s["c_prev"] if mutate == "c_in unmasked in dz_f" else s["c_in"]) * s["df"],
                             dc * s["i"] * ((1 - s["g"]) if mutate == "wrong g derivative" else s["dg"]),
                             do * s["do"]])
        oph = s["hhead"] if mutate == "gWh against h_t" else s["oph"]
        gWg += dz @ np.concatenate([s["opx"], oph]).T
        gWhd += Dt @ s["hhead"].T
        gbh += Dt.sum(axis=1)
        cut = np.zeros(E, bool) if mutate == "not cut at starts" else s["start"]
        dh_next = np.where(cut, 0.0, s["Wg"][:, F + 2:].T @ dz)
        dc_next = np.where(cut, 0.0, dc * s["f"])
    div = float(T * n) if mutate == "divisor T n" else float(B)
    grads = dict(wx=gWg[:, :F], wt=gWg[:, F:F + 1], b=gWg[:, F + 1:F + 2], wh=gWg[:, F + 2:], w2=gWhd[:-1],
                 b2=gbh[:-1].reshape(-1, 1), wv=gWhd[-1:], bv=gbh[-1:].reshape(1, 1))
    grads = {k: np.ascontiguousarray(v) / div for k, v in grads.items()}
    pol = -(np.minimum(t1, t2) * k1).sum() / B
    val = (((ret - value) ** 2) * k1).sum() / B
    entl = -(H_all * k1).sum() / B
    stats = dict(policy_loss=pol, value_loss=val, entropy_loss=entl, approx_kl=((old - lp0) * k1).sum() / B,
                 clip_fraction=((np.abs(ratio - 1) > hp.clip) & good).sum() / B,
                 grad_norm=float(np.sqrt(sum((g ** 2).sum() for g in grads.values()))),
                 adv_mean=mean, adv_std=std, bad=float((~good).sum()), loss=pol + hp.ent * entl + hp.vf * val)
    inter = dict(steps=steps, lp=np.where(good, lp, -np.inf).reshape(T, E), value=value.reshape(T, E), D=D, good=good,
                 ratio=ratio)
    return grads, stats, inter


def rel_diff(got, ref):
    """Per tensor max |got - ref| / max |ref|."""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k]).max() / np.abs(ref[k]).max())
            for k in ref}


def stats_diff(got, ref, names=STATS):
    """Per statistic |got - ref| / max(1, |ref|)."""
    return {k: abs(float(got[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in names}


def mutant_moves(case, hp):
    """{mutant: the largest relative move (``rel_diff``) it causes in any tensor of the emulated gradient}."""
    ref, _, inter = loss_and_grad(case, hp, emulate=True)
    return {m: max(rel_diff(loss_and_grad(case, hp, emulate=True, mutate=m, steps=inter["steps"])[0], ref).values())
            for m in MUTANTS}


# ---- the shared inputs ---------------------------------------------------------------------------------------------
def make_case(T, n, envs, F, C, odt, seed, scale=1, starts=(), bad=()):
    """A synthetic full sink of T slots and n envs and a minibatch ``envs`` of it.  Rows from recurrent_ref.make_rows,
    the module from make_module; the recorded log-probs are the emulated current ones moved by +-0.05 or +-0.4
    (rho near 0.95, 1.05, 0.67, 1.49: both clip sides occur, and no sample sits within rounding of a clip
    edge, where PPO's gradient is discontinuous).  ``starts``: steps t at which about a third of the envs start
    an episode (others: none); ``bad``: (t, env, head) whose recorded action is out of range."""
    rng = np.random.default_rng(7000 + seed)
    pol = rr.make_module(F, C, seed, scale)
    obs = np.stack([rr.make_rows(F, n, odt, seed + 13 * t) for t in range(T)])
    ts = rng.integers(0, 334, (T, n)) / 333.0
    actions = np.stack([rng.integers(0, 4, (T, n)), rng.integers(0, C, (T, n))], axis=1).astype(np.int32)
    es = np.zeros((T, n), np.float32)
    for t in starts:
        es[t] = (rng.random(n) < 0.35).astype(np.float32)
        es[t, np.asarray(envs)[0]] = 1.0
    adv = rng.normal(0.0, 1.5, (T, n)).astype(np.float32)
    ret = rng.normal(0.0, 1.0, (T, n)).astype(np.float32)
    h0 = rng.uniform(-1, 1, (H, n)).astype(np.float32)
    c0 = rng.uniform(-1, 1, (H, n)).astype(np.float32)
    case = dict(T=T, n=n, F=F, C=C, odt=odt, pol=pol, w=rr.weights(pol), obs=obs, ts=ts, actions=actions, es=es, adv=adv,
                ret=ret, h0=h0, c0=c0, envs=np.arange(n, dtype=np.int32), old_lp=np.zeros((T, n), np.float32))
    lp = loss_and_grad(case, test_hp())[2]["lp"]                            # over every env of the sink
    delta = rng.choice([-0.4, -0.05, 0.05, 0.4], (T, n)) * rng.uniform(0.9, 1.1, (T, n))
    case["old_lp"] = (lp - delta).astype(np.float32)
    for t, e, head in bad:
        case["actions"][t, head, e] = 4 + C
    case["envs"] = np.asarray(envs, np.int32)
    return case


def cpu_case():
    """T = 6, n = 9, every env once, starts at t = 0, at mid-sequence and at the last step."""
    return make_case(6, 9, np.arange(9), 29, 5, "float32", 3, starts=(0, 3, 5))


def gpu_cases():
    """The cases a, b, c of tests/test_recurrent_ppo_gpu.py: (name, case)."""
    rng = np.random.default_rng(99)
    eb = rng.permutation(40)[:33]
    ec = rng.permutation(100)[:95]
    ec = np.concatenate([ec, ec[:1]])                                        # one repeat
    return [("a", make_case(1, 32, [5, 5], 14, 1, "int8", 11)),
            ("b", make_case(2, 40, eb, 29, 5, "int32", 12)),
            ("c", make_case(7, 100, ec, 62, 16, "float32", 13, scale=2, starts=(0, 3, 6)))]


def edge_cases():
    """The cases d, e, e48, f, g: the paths a full-size minibatch takes that a-c do not reach: (name, case).

        d    T = 52, n = 136, 128 envs permuted + one repeat (E = 129, 5 tiles), F 30, C 3, int8, starts at t = 0, 1, 2,
             17, 51: 260 (t, tile) items -- the default plan is 256 workgroups of 2 rounds, the second with 4 live
             items; int8 rows beyond t = 0; F + 2 = 32, one full x tile; BPTT through 52 steps
        e    T = 3, n = 40, 33 envs, F 31, C 2, int32, start at t = 1: F + 2 = 33, a second x tile with one live column
        e48  e with F = 46: F + 2 = 48, three full x k-steps
        f    T = 3, n = 40, 32 envs, F 15, C 1, int8, start at t = 2: F + 2 = 17; no idle lane; int8 rows at t = 1, 2
        g    T = 6, n = 36, envs [7], F 47, C 7, float32, start at t = 2: F + 2 = 49; E = 1, 31 clamped lanes
    """
    rng = np.random.default_rng(77)
    ed = rng.permutation(136)[:128]
    ed = np.concatenate([ed, ed[:1]])                                        # one repeat
    ee = rng.permutation(40)[:33]
    ef = rng.permutation(40)[:32]
    return [("d", make_case(52, 136, ed, 30, 3, "int8", 14, starts=(0, 1, 2, 17, 51))),
            ("e", make_case(3, 40, ee, 31, 2, "int32", 15, starts=(1,))),
            ("e48", make_case(3, 40, ee, 46, 2, "int32", 18, starts=(1,))),
            ("f", make_case(3, 40, ef, 15, 1, "int8", 16, starts=(2,))),
            ("g", make_case(6, 36, [7], 47, 7, "float32", 17, starts=(2,)))]


LONG = ("d",)                            # the cases TOL_G_LONG / TOL_S_LONG are for


def tolerances(name):
    """(gradient, statistics) tolerance of the case ``name``."""
    return (TOL_G_LONG, TOL_S_LONG) if name in LONG else (TOL_G, TOL_S)
