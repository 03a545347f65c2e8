"""A float64 restatement of the PPO update (include/oc_policy.h: oc_policy_ppo_update / oc_policy_ppo_grad) for the
tests -- not a test module.  Like tests/policy_ref.py and tests/policy_ac_ref.py, on which it builds,
it is written from the module's plain weights and the header's definitions, never from the packed
fragments.

    loss_and_grad(case, hp, emulate, mutate)   the loss terms, the ten statistics' raw values and the
                                               UNCLIPPED gradient of the seven tensors
    clip(grads, max_norm)                      clip_grad_norm_
    adam(w, m, v, g, t, ...)                   torch's Adam, amsgrad False, no weight decay
    grad_bound(case, hp, plan)                 how far the kernel's clipped gradient and statistics may
                                               lie from loss_and_grad(emulate=True) + clip
    adam_bound(...)                            how far its float32 Adam may lie from adam()
    make_case(...)                             the inputs the GPU tests and the mutation tests share

``emulate=True`` evaluates the gradient where the header says the kernel does: at the network the
fragments represent (``policy_ref._forward``), with h = 1 - 2 r and tanh' = 4 r (1 - r) from the
unrounded r, and the roundings not differentiated.  ``emulate=False`` is the exact module.
"""
import numpy as np

import policy_ac_ref as ar
import policy_ref as pr

U = pr.U_F32
NAMES = ("w1", "wt", "b1", "w2", "b2", "wv", "bv")
STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm",
         "adv_mean", "adv_std", "bad", "loss")
MUTATIONS = ("drop_sample", "ent_zero", "no_clip_mask", "vf_half", "biased_std", "one_minus_h")
ADAM_MUTATIONS = ("no_bias_correction", "eps_in_root", "no_clip_coef")


def f32(x):
    """The float32 value of a hyper-parameter, as the kernel receives it."""
    return float(np.float32(x))


class HP:
    """The hyper-parameters as the kernel sees them: float32 values."""

    def __init__(self, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, lr=3e-4,
                 betas=(0.9, 0.999), eps=1e-5):
        self.clip, self.ent, self.vf, self.max_norm = f32(clip_range), f32(ent_coef), f32(vf_coef), f32(max_grad_norm)
        self.lr, self.b1, self.b2, self.eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)


# ---- the network and its intermediates ---------------------------------------------------------
def _network(w, wv, bv, rows, ts, emulate):
    """x [F + 2][n], h [64][n], logits [4 + C][n] (natural), value [n], the rows [w2; wv] the backward
    multiplies by, and (emulate) policy_ref's intermediates."""
    sw = ar.stack(w, wv, bv)
    if emulate:
        f = pr._forward(*sw, rows, ts)
        out = f["L2"] * pr.LN2
        # tanh' as the header writes it, 4 r (1 - r): 1 - h^2 would cancel in float64 where r < 1e-12
        return dict(x=f["X"], h=1.0 - 2.0 * f["r"], dact=4.0 * f["r"] * (1.0 - f["r"]), logits=out[:-1],
                    value=out[-1], W2=f["W2h"] * (-pr.LN2 / 2.0), f=f)
    x = np.concatenate([np.asarray(rows).astype(np.float64), np.asarray(ts, np.float64).reshape(1, -1),
                        np.ones((1, np.asarray(rows).shape[1]))], axis=0)
    w1, wt, b1, w2s, b2s = (np.asarray(a, np.float64) for a in sw)
    h = np.tanh(np.concatenate([w1, wt.reshape(-1, 1), b1.reshape(-1, 1)], axis=1) @ x)
    out = w2s @ h + b2s.reshape(-1, 1)
    return dict(x=x, h=h, dact=1.0 - h * h, logits=out[:-1], value=out[-1], W2=w2s, f=None)


def _heads(logits, actions):
    """Per head: (rows lo:hi, p [K][n], ln p [K][n], H [n], one-hot [K][n], in-range [n])."""
    out = []
    n = logits.shape[1]
    for col, (lo, hi) in enumerate(ar.HEADS):
        L = logits[lo:hi]
        ls = ar.head_log_softmax(L)
        p = np.exp(ls)
        H = -(p * ls).sum(axis=0)
        a = np.asarray(actions)[:, col].astype(np.int64)
        ok = (a >= 0) & (a < L.shape[0])
        hot = np.zeros_like(L)
        hot[a[ok], np.arange(n)[ok]] = 1.0
        out.append((lo, lo + L.shape[0], p, ls, H, hot, ok))
    return out


def loss_and_grad(case, hp, emulate=True, mutate=None):
    """The header's loss and its gradient over the B samples of ``case`` (make_case: the gathered
    minibatch), in float64.  Returns (grads {name: array}, stats {name: value}, intermediates).
    ``mutate`` plants one of MUTATIONS (the tests' check that the bounds are not vacuous)."""
    net = _network(case["w"], case["wv"], case["bv"], case["rows"], case["ts"], emulate)
    adv, ret, old = (np.asarray(case[k], np.float64) for k in ("adv", "ret", "old_lp"))
    B = adv.shape[0]
    F = np.asarray(case["w"][0]).shape[1]
    ent = 0.0 if mutate == "ent_zero" else hp.ent
    vf = 0.5 * hp.vf if mutate == "vf_half" else hp.vf
    mean, std = adv.mean(), adv.std(ddof=0 if mutate == "biased_std" else 1)
    ahat = (adv - mean) / (std + 1e-8)
    heads = _heads(net["logits"], case["actions"])
    good = heads[0][6] & heads[1][6]
    keep = good.astype(np.float64)
    lp = np.zeros(B)
    for lo, hi, p, ls, H, hot, ok in heads:
        lp += (ls * hot).sum(axis=0)
    lp = np.where(good, lp, -np.inf)
    ratio = np.where(good, np.exp(np.where(good, lp, 0.0) - old), 0.0)
    t1 = ahat * ratio
    t2 = ahat * np.clip(ratio, 1 - hp.clip, 1 + hp.clip)
    inside = (ratio >= 1 - hp.clip) & (ratio <= 1 + hp.clip)
    through = np.ones(B, bool) if mutate == "no_clip_mask" else ((t1 <= t2) | inside)
    glp = np.where(through, -t1, 0.0)
    D = np.zeros((net["W2"].shape[0], B))                    # d (B loss) / d [logits; value]
    H_all = np.zeros(B)
    for lo, hi, p, ls, H, hot, ok in heads:
        D[lo:hi] = glp * (hot - p) + ent * p * (ls + H)
        H_all += H
    D[-1] = 2.0 * vf * (net["value"] - ret)
    D *= keep
    h, x, W2 = net["h"], net["x"], net["W2"]
    if mutate == "drop_sample":
        # a sample that contributes nothing to a tensor (saturated units, a clipped ratio) can be lost
        # without a trace there, so the one dropped is the one that carries the most weight in all three
        # groups of tensors: the first layer (through dpre), the logit rows, the value row
        share = lambda a: a / max(a.sum(), 1e-300)  # noqa: E731
        pre = np.abs((W2.T @ D) * net["dact"]).sum(axis=0)
        lose = np.argmax(np.minimum(np.minimum(share(pre), share(np.abs(D[:-1]).sum(axis=0))), share(np.abs(D[-1]))))
        D[:, lose] = 0.0
    dW2 = D @ h.T / B
    db2 = D.sum(axis=1) / B
    dh = W2.T @ D
    dpre = dh * ((1.0 - h) if mutate == "one_minus_h" else net["dact"])
    dW1 = dpre @ x.T / B
    shapes = dict(w1=(64, F), wt=(64, 1), b1=(64, 1), w2=(D.shape[0] - 1, 64), b2=(D.shape[0] - 1, 1), wv=(1, 64),
                  bv=(1, 1))
    grads = dict(w1=dW1[:, :F], wt=dW1[:, F], b1=dW1[:, F + 1], w2=dW2[:-1], b2=db2[:-1], wv=dW2[-1], bv=db2[-1:])
    grads = {k: np.asarray(v, np.float64).reshape(shapes[k]) for k, v in grads.items()}
    k1 = good.astype(np.float64)
    pol = -(np.minimum(t1, t2) * k1).sum() / B
    val = (((ret - net["value"]) ** 2) * k1).sum() / B
    entl = -(H_all * k1).sum() / B
    stats = dict(policy_loss=pol, value_loss=val, entropy_loss=entl,
                 approx_kl=(np.where(good, old - np.where(good, lp, 0.0), 0.0)).sum() / B,
                 clip_fraction=((np.abs(ratio - 1) > hp.clip) & good).sum() / B,
                 grad_norm=float(np.sqrt(sum((g ** 2).sum() for g in grads.values()))),
                 adv_mean=mean, adv_std=std, bad=float((~good).sum()), loss=pol + hp.ent * entl + hp.vf * val)
    inter = dict(net=net, heads=heads, good=good, keep=keep, ahat=ahat, lp=lp, ratio=ratio, t1=t1, t2=t2, glp=glp,
                 D=D, dh=dh, dpre=dpre, mean=mean, std=std, inside=inside, H=H_all)
    return grads, stats, inter


def clip(grads, max_norm):
    """clip_grad_norm_: (clipped grads, norm, coefficient)."""
    norm = float(np.sqrt(sum((g ** 2).sum() for g in grads.values())))
    coef = min(1.0, max_norm / (norm + 1e-6))
    return {k: g * coef for k, g in grads.items()}, norm, coef


def adam(w, m, v, g, t, hp, mutate=None):
    """Step t (1-based) of torch.optim.Adam (amsgrad False, no weight decay) on float64 arrays."""
    m2 = hp.b1 * m + (1 - hp.b1) * g
    v2 = hp.b2 * v + (1 - hp.b2) * g * g
    bc1, bc2 = (1.0, 1.0) if mutate == "no_bias_correction" else (1 - hp.b1 ** t, 1 - hp.b2 ** t)
    if mutate == "eps_in_root":
        denom = np.sqrt(v2 / bc2 + hp.eps)
    else:
        denom = np.sqrt(v2) / np.sqrt(bc2) + hp.eps
    return w - (hp.lr / bc1) * (m2 / denom), m2, v2


# ---- bounds ------------------------------------------------------------------------------------
def _g(k):
    return pr._gamma(k)


def grad_bound(case, hp, plan):
    """Bounds on |kernel - reference| for the CLIPPED gradient of each tensor and for the ten
    statistics, where the reference is clip(loss_and_grad(case, hp, emulate=True)).
    ``plan`` = (G, tiles per wave, ...) of oc_policy_ppo_plan.  Returns ({name: bound array} for the UNCLIPPED
    gradient, {stat: bound}, the reference's unclipped gradient, its statistics); ``clipped_check``
    compares a clipped gradient.

    Every fp32 operation is charged u = 2^-23 (policy_ref.U_F32), a k-term fp32 sum gamma(k).  The
    derivation follows the kernel, operation by operation:

    forward      the logits and the value are within policy_ref.logit_bound (lb, per row) of the
                 emulated ones, lp within policy_ac_ref.log_prob_bound (lpb); r within logit_bound's
                 `window` of the exact r.
    A^           mean and std come from double sums, rounded to float (u each); then a subtraction, an
                 addition of 1e-8 and a division:  e_A = u |mean| / den + 5 u |A^|.
    rho          = expf(lp - old): the argument is off by lpb + u |lp - old|, expf by 2 ulp:
                 e_rho = rho (expm1(lpb + u |lp - old|) + 2 u).
    -A^ rho      e_t = |A^| e_rho + rho e_A + e_A e_rho + u |t|.  The clip decision compares rho with
                 1 -+ c (each a float subtraction, u) and A^ rho with A^ clamp(rho): a sample whose rho
                 lies within e_rho + 2 u of a clip edge, or whose |A^| <= e_A, may be decided the other
                 way and is charged its whole term |t| (as logit_bound charges a flipped rounding).
    p, ln p      (for the statistics; d logits takes the logits' error through its Jacobian, see the code)
                 per head, with mlb the head's largest lb: the softmax moves by at most a factor
                 exp(+-2 mlb); its own arithmetic is log_prob_bound's (exp2 terms u e + 0.37 u each,
                 the total rel_S, a division and a product):
                 e_p = p (expm1(2 mlb) + rel_S + 4 u) + 0.37 u;
                 e_lnp = lb_c + mlb + ln 2 (u |d_c| + u max(|log2 S|, 1) + rel_S / (ln 2 (1 - rel_S)) + u |q_c|)
                         + 2 u |ln p_c|, the magnitudes enlarged by (lb_c + mlb) / ln 2 as in log_prob_bound;
                 e_H = sum_c (e_p |ln p| + p e_lnp + e_p e_lnp) + gamma(2 K) sum_c |p ln p|.
    d logits     glp (1[c = a] - p_c) + ent p_c (ln p_c + H): products and sums of the above, 4 more
                 operations (4 u of the result's terms).  d v = 2 vf (v - ret): 2 vf lb_v + 3 u |d v|.
    dh           32 fp32 multiply-adds per element (16 k-steps of 2 rows; unused rows are exact zeros):
                 e_dh = gamma(33) |W2'|^T |d| + |W2'|^T e_d   (in the folded weights' units).
    dpre         = (-2 ln 2) dh (r (1 - r)):  s = r (1 - r) moves by window |1 - 2 r| + window^2 and
                 costs 2 u;  e_dpre = 2 ln 2 (e_dh (s + e_s) + |dh| e_s) + 4 u |dpre|.
    h            = 1 - 2 r:  e_h = 2 window + u |h|.
    sums over    a wave adds 32 samples per tile over its tiles (K1 = 32 tiles_per_wave multiply-adds,
    samples      charged K1 + 2), the workgroup adds its 4 waves, the finish adds G partials and divides
                 by B:  K = 32 tpw + 2 + 4 + G + 1;  for a gradient element sum_s a_s b_s / B:
                 gamma(K) sum |a| |b| / B + sum (e_a |b| + |a| e_b + e_a e_b) / B.   (x is exact.)
    clip         see the end of the function and ``clipped_check``.
    """
    grads, stats, it = loss_and_grad(case, hp, emulate=True)
    net, f = it["net"], it["net"]["f"]
    w, wv, bv, rows, ts = case["w"], case["wv"], case["bv"], case["rows"], case["ts"]
    B = it["ahat"].shape[0]
    F = np.asarray(w[0]).shape[1]
    G, tpw = int(plan[0]), int(plan[1])
    lb, info = pr.logit_bound(*ar.stack(w, wv, bv), rows, ts)          # [5 + C][n], value last
    lpb = ar.log_prob_bound(w, rows, ts, np.clip(np.asarray(case["actions"]), 0, None))
    window = info["window"]
    good, keep = it["good"], it["keep"]
    old = np.asarray(case["old_lp"], np.float64)
    lp0 = np.where(good, it["lp"], 0.0)
    ahat, ratio = it["ahat"], it["ratio"]
    den = it["std"] + 1e-8
    e_A = U * abs(it["mean"]) / den + 5 * U * np.abs(ahat)
    e_rho = ratio * (np.expm1(lpb + U * np.abs(lp0 - old)) + 2 * U)
    t = np.abs(it["t1"])
    e_t = np.abs(ahat) * e_rho + ratio * e_A + e_A * e_rho + U * t
    edge = np.minimum(np.abs(ratio - (1 - hp.clip)), np.abs(ratio - (1 + hp.clip)))
    marginal = (edge <= e_rho + 2 * U) | (np.abs(ahat) <= e_A)
    e_glp = np.where(marginal, t + e_t, e_t)
    glp = np.abs(it["glp"])
    glp_max = np.where(marginal, t, glp)

    # d logits: the logits' own error goes through the JACOBIAN of d with respect to the logits (both
    # heads: rho depends on both), which keeps the signs the per-quantity bounds above would lose --
    #   d pol_o / d L_c = glp (1[c = a] - p_c)(1[o = a] - p_o) - [same head] glp p_o (1[o = c] - p_c)
    #   d ent_o / d L_c = [same head] ent p_o ((1[o = c] - p_c)(ln p_o + H + 1) - p_c (ln p_c + H))
    # evaluated at the reference and enlarged by exp(4 sum of the heads' largest lb) for its own
    # variation inside the box; the float32 arithmetic behind the kernel's logits is charged
    # separately with the formulas above and lb = 0 (log_prob_bound's `arith`).
    D = np.abs(it["D"])
    e_D = np.zeros_like(D)
    e_H_all = np.zeros(B)
    nl = net["logits"].shape[0]
    hotp = np.zeros((nl, B))
    pall = np.zeros((nl, B))
    lsH = np.zeros((nl, B))
    head_of = np.zeros(nl, np.int64)
    mlb_sum = np.zeros(B)
    part = np.zeros(B)
    for hd, (lo, hi, p, ls, H, hot, ok) in enumerate(it["heads"]):
        hotp[lo:hi], pall[lo:hi], lsH[lo:hi], head_of[lo:hi] = hot - p, p, ls + H, hd
        mlb_sum += lb[lo:hi].max(axis=0)
        a_idx = np.clip(np.asarray(case["actions"])[:, hd].astype(np.int64), 0, hi - lo - 1)
        part += lb[lo:hi][a_idx, np.arange(B)] + lb[lo:hi].max(axis=0)
    arith_lp = lpb - part                                      # log_prob_bound without the logits' part
    same = (head_of[:, None] == head_of[None, :]).astype(np.float64)[:, :, None]          # [o][c][1]
    eye = np.eye(nl)[:, :, None]
    g_signed = it["glp"][None, None, :]
    J = g_signed * hotp[None, :, :] * hotp[:, None, :] - same * g_signed * pall[:, None, :] * (eye - pall[None, :, :])
    J = J + same * hp.ent * pall[:, None, :] * ((eye - pall[None, :, :]) * (lsH[:, None, :] + 1.0)
                                                  - pall[None, :, :] * lsH[None, :, :])
    e_jac = (np.abs(J) * lb[None, :nl, :]).sum(axis=1) * np.exp(4 * mlb_sum)
    # the arithmetic part: rho's, A^'s and the clip decision's share of glp
    e_rho_a = ratio * (np.expm1(arith_lp + U * np.abs(lp0 - old)) + 2 * U)
    e_t_a = np.abs(ahat) * e_rho_a + ratio * e_A + e_A * e_rho_a + U * t
    e_glp_a = np.where(marginal, t + e_t, e_t_a)
    for lo, hi, p, ls, H, hot, ok in it["heads"]:
        K = hi - lo
        b = lb[lo:hi]
        mlb = b.max(axis=0)
        L2 = net["logits"][lo:hi] / pr.LN2
        slack = (b + mlb) / pr.LN2
        d = np.abs(L2 - L2.max(axis=0)) + slack
        S = np.exp2(L2 - L2.max(axis=0)).sum(axis=0)
        g = np.abs(np.log2(S)) + slack
        rel_S = _g(K - 1) + U + K * (0.37 * U + 2.0 ** -126)
        q = d + g
        ar_p = p * (rel_S + 4 * U) + 0.37 * U
        ar_lnp = pr.LN2 * (U * d + U * np.maximum(g, 1.0) + rel_S / (pr.LN2 * (1 - rel_S)) + U * q) \
            + 2 * U * (np.abs(ls) + b + mlb)
        e_p = p * np.expm1(2 * mlb) + ar_p                     # (for the entropy statistic)
        e_lnp = b + mlb + ar_lnp
        e_H_all += (e_p * np.abs(ls) + p * e_lnp + e_p * e_lnp).sum(axis=0) + _g(2 * K) * np.abs(p * ls).sum(axis=0)
        ar_H = (ar_p * np.abs(ls) + p * ar_lnp + ar_p * ar_lnp).sum(axis=0) + _g(2 * K) * np.abs(p * ls).sum(axis=0)
        lH = np.abs(ls + H)
        pol = np.abs(hot - p)
        e_pol = e_glp_a * pol + (glp_max + e_glp_a) * (ar_p + U) + U * glp_max * pol
        e_ent = hp.ent * (ar_p * lH + (p + ar_p) * (ar_lnp + ar_H + U * lH)) + 2 * U * hp.ent * p * lH
        e_D[lo:hi] = e_jac[lo:hi] + e_pol + e_ent + 4 * U * (glp_max * pol + hp.ent * p * lH)
    dv = np.abs(2 * hp.vf * (net["value"] - np.asarray(case["ret"], np.float64)))
    e_D[-1] = 2 * hp.vf * lb[-1] + 3 * U * dv
    e_D *= good                                               # a bad sample's d is an exact zero
    Dk = D

    W2f = np.abs(f["W2h"])                                    # folded units
    dh_f = np.abs(it["dh"]) / (pr.LN2 / 2.0)
    e_dh = _g(33) * (W2f.T @ (Dk + e_D)) + W2f.T @ e_D
    r = f["r"]
    s = r * (1 - r)
    e_s = window * np.abs(1 - 2 * r) + window ** 2 + 2 * U * s
    dpre = np.abs(it["dpre"])
    e_dpre = 2 * pr.LN2 * (e_dh * (s + e_s) + dh_f * e_s) + 4 * U * dpre
    h = np.abs(net["h"])
    e_h = 2 * window + U * h
    x = np.abs(net["x"])

    Ks = 32 * tpw + 2 + 4 + G + 1
    e_dW2 = (_g(Ks) * ((Dk + e_D) @ (h + e_h).T) + e_D @ h.T + Dk @ e_h.T + e_D @ e_h.T) / B
    e_db2 = (_g(Ks) * (Dk + e_D).sum(axis=1) + e_D.sum(axis=1)) / B
    e_dW1 = (_g(Ks) * ((dpre + e_dpre) @ x.T) + e_dpre @ x.T) / B
    raw = dict(w1=e_dW1[:, :F], wt=e_dW1[:, F], b1=e_dW1[:, F + 1], w2=e_dW2[:-1], b2=e_db2[:-1], wv=e_dW2[-1],
               bv=e_db2[-1:])
    raw = {k: np.asarray(v).reshape(grads[k].shape) for k, v in raw.items()}

    # the clip: the kernel's coefficient comes from ITS norm (reported in the statistics), so the
    # elementwise check is made against the reference's unclipped gradient times that coefficient
    # (clipped_check below) and the norm is checked on its own: a double sum of float squares,
    # |norm(g + e) - norm(g)| <= min(|e|_2, (sum |g| e + |e|_2^2 / 2) / norm), plus the rounding to float
    norm = stats["grad_norm"]
    e2 = float(np.sqrt(sum((v ** 2).sum() for v in raw.values())))
    first = (sum((np.abs(grads[k]) * raw[k]).sum() for k in raw) + 0.5 * e2 * e2) / max(norm, 1e-300)
    e_norm = min(e2, first) + U * norm
    bound = raw

    k1 = good.astype(np.float64)
    acc = (tpw + 3) * U                                       # a lane's float sums over its tiles, the product, the store
    val_d = np.abs(np.asarray(case["ret"], np.float64) - net["value"])
    sb = dict(
        policy_loss=((np.where(marginal, t + e_t, e_t) + acc * t) * k1).sum() / B,
        value_loss=((2 * val_d * lb[-1] + lb[-1] ** 2 + (3 * U + acc) * val_d ** 2) * k1).sum() / B,
        entropy_loss=((e_H_all + acc * np.abs(it["H"])) * k1).sum() / B,
        approx_kl=((lpb + (U + acc) * np.abs(old - lp0)) * k1).sum() / B,
        clip_fraction=float(((np.abs(np.abs(ratio - 1) - hp.clip) <= e_rho + 3 * U) & good).sum()) / B,
        grad_norm=e_norm, adv_mean=U * abs(it["mean"]) + 1e-30, adv_std=2 * U * it["std"], bad=0.0)
    sb["loss"] = sb["policy_loss"] + hp.ent * sb["entropy_loss"] + hp.vf * sb["value_loss"] + U * (
        abs(stats["policy_loss"]) + hp.ent * abs(stats["entropy_loss"]) + hp.vf * abs(stats["value_loss"]))
    return bound, sb, grads, dict(stats, marginal=int((marginal & good).sum()))


def clipped_check(got, kernel_norm, ref, bound, hp):
    """Whether a clipped gradient `got` {name: array} is the reference's unclipped one times the
    coefficient min(1, max_norm / (kernel_norm + 1e-6)) within the bound: the coefficient is three
    float32 operations (3 u), the product one more.  Returns the largest excess over the bound
    (<= 0: inside) per tensor."""
    return {k: v[0] for k, v in clipped_excess(got, kernel_norm, ref, bound, hp).items()}


def clipped_excess(got, kernel_norm, ref, bound, hp):
    """clipped_check with the element of the largest excess: {name: (excess, got, reference, bound)}."""
    coef = min(1.0, hp.max_norm / (kernel_norm + 1e-6))
    out = {}
    for k in ref:
        g = np.asarray(got[k], np.float64).reshape(ref[k].shape)
        want, tol = ref[k] * coef, bound[k] * coef + 4 * U * np.abs(ref[k]) * coef
        ex = np.abs(g - want) - tol
        at = np.unravel_index(np.argmax(ex), ex.shape)
        out[k] = (float(ex[at]), float(g[at]), float(want[at]), float(tol[at]))
    return out


def adam_bound(w, m, v, g, t, hp):
    """Bounds (e_w, e_m, e_v) on |kernel - adam()| for a step from the SAME state and gradient (float32
    values), the kernel working in float32:

        m' = b1 m + (1 - b1) g        1 - b1 is a float subtraction (u), two products, one sum:
                                      e_m = 3 u (|b1 m| + |(1 - b1) g|)
        v' = b2 v + (1 - b2) g g      one product more:  e_v = 4 u (|b2 v| + |(1 - b2) g g|)
        bc1, sqrt(bc2)                formed in double, rounded to float: u each
        denom = sqrt(v') / sqrt(bc2) + eps    sqrt halves v's relative error (2 u), then sqrt, the
                                      division, bc2's rounding and the sum: 6 u of denom
        upd = (lr / bc1) (m' / denom) lr / bc1: 2 u;  the division and the product: 2 u;  m' enters
                                      with its absolute error:  e_upd = 10 u |upd| + (lr / bc1) e_m / denom
        w' = w - upd                  e_w = e_upd + u |w'|
    """
    w2, m2, v2 = adam(w, m, v, g, t, hp)
    e_m = 3 * U * (np.abs(hp.b1 * m) + np.abs((1 - hp.b1) * g))
    e_v = 4 * U * (np.abs(hp.b2 * v) + np.abs((1 - hp.b2) * g * g))
    bc1, bc2 = 1 - hp.b1 ** t, 1 - hp.b2 ** t
    denom = np.sqrt(v2) / np.sqrt(bc2) + hp.eps
    upd = (hp.lr / bc1) * (m2 / denom)
    e_w = 10 * U * np.abs(upd) + (hp.lr / bc1) * e_m / denom + U * np.abs(w2)
    return e_w, e_m, e_v


# ---- the shared inputs ---------------------------------------------------------------------------
T_SLOTS, N_ENVS = 3, 70
# (F, C, obs type, weight scale, B, max_groups, seed): a thin cover of F in {14, 30, 31, 46} (k-steps 1, 2
# exactly full, 3, the maximum), C in {1, 3, 16}, the three obs types, B in {2, 32, 33, 210, 300} and
# max_groups in {0, 1, 3} (210 samples in one workgroup: two tiles per wave; 300: three).
# The seeds: PPO's gradient is discontinuous where rho crosses a clip edge, so a sample whose rho lies
# within its own error of 1 -+ c is charged its whole term by grad_bound (`marginal`), and one such
# sample swamps every small mutation in the small tensors; with errors of 1e-4 .. 1e-3 in rho and 210
# samples that happens in every second buffer.  Each seed is the first from F + C on for which the
# buffer has no such sample and every planted mutation of tests/test_ppo_ref_cpu.py is visible (for
# B = 2 that needs one of the two samples clipped away).
GRAD_CASES = [(14, 1, "int32", 1, 210, 0, 16), (30, 3, "int8", 4, 33, 1, 33), (31, 16, "float32", 1, 300, 3, 48),
              (46, 3, "float32", 4, 210, 1, 52), (46, 16, "int32", 1, 32, 0, 62), (30, 1, "int8", 1, 2, 0, 33),
              (14, 3, "int8", 1, 300, 1, 17), (31, 3, "int32", 4, 210, 3, 37)]


def test_hp():
    """The hyper-parameters of the gradient and apply tests: an entropy term that matters, a norm clip
    that is active, and a step large enough to show next to one float32 ulp of the largest weight."""
    return HP(ent_coef=0.01, max_grad_norm=0.05, lr=3e-3)


def ref_plan(B, max_groups):
    """oc_policy_ppo_plan's (G, tiles per wave), restated: at most one tile per wave up to the cap (64 by default)."""
    tiles = (B + 31) // 32
    G = min((tiles + 3) // 4, max_groups if max_groups > 0 else 64)
    return G, (tiles + 4 * G - 1) // (4 * G)


def make_buffer(F, C, odt, scale, seed):
    """The synthetic rollout the GPU tests record: T = 3 slots of n = 70 envs (210 samples, no multiple
    of 32).  Rows from policy_ac_ref.make_rows, weights from make_actor_critic; the recorded log-probs
    come from slightly different weights (the `old` module: every weight scaled by 0.97 and w2 nudged),
    so that rho != 1 and both clip sides occur; advantages carry a constant-sign block (slot 0 all
    positive).  Returns a dict of numpy arrays and the two torch modules (CPU)."""
    import torch
    T, n = T_SLOTS, N_ENVS
    rng = np.random.default_rng(4242 + seed)
    obs = np.stack([ar.make_rows(F, n, odt, seed + 11 * s) for s in range(T)])            # [T][F][n]
    ts = np.stack([ar.make_timesteps(n, 100, seed + s) for s in range(T)])               # [T][n]
    actions = np.stack([rng.integers(0, 4, (T, n)), rng.integers(0, C, (T, n))], axis=1).astype(np.int32)   # [T][2][n]
    pol = ar.make_actor_critic(F, C, seed, scale)
    old = ar.make_actor_critic(F, C, seed, scale)
    g = torch.Generator().manual_seed(77 + seed)
    with torch.no_grad():
        for t_ in (old.w1, old.b1, old.wt, old.w2, old.b2, old.wv, old.bv):
            t_.mul_(0.97)
        old.w2.add_(0.3 * scale / 8.0 * (torch.rand(old.w2.shape, generator=g) * 2 - 1))
    adv = rng.normal(0.0, 1.5, (T, n))
    adv[0] = np.abs(adv[0]) + 0.25
    ret = rng.normal(0.0, 1.0, (T, n))
    return dict(obs=obs, ts=ts, actions=actions, adv=adv.astype(np.float32), ret=ret.astype(np.float32), pol=pol,
                old=old, F=F, C=C, odt=odt)


def old_log_probs(buf):
    """The recorded log-probs [T][n] as the float64 emulation of the `old` module gives them (the GPU
    tests record score()'s instead: the same to a few float32 ulps)."""
    w, wv, bv = ar.weights(buf["old"])
    T = buf["obs"].shape[0]
    return np.stack([ar.ref_log_prob(w, buf["obs"][s], buf["ts"][s], buf["actions"][s].T)[0]
                     for s in range(T)]).astype(np.float32)


def make_indices(B, seed=0):
    """The minibatches the tests use, over the 210 samples: 2, 32, 33 (the first ones shuffled), 210 (a
    permutation), 300 (with repeats)."""
    total = T_SLOTS * N_ENVS
    rng = np.random.default_rng(900 + B + seed)
    if B <= total:
        return rng.permutation(total)[:B].astype(np.int32)
    return rng.integers(0, total, B).astype(np.int32)


def make_case(buf, idx, old_lp, pol=None):
    """The minibatch `idx` gathered from a buffer: what loss_and_grad / grad_bound take."""
    w, wv, bv = ar.weights(pol if pol is not None else buf["pol"])
    n = buf["obs"].shape[2]
    idx = np.asarray(idx, np.int64)
    slot, env = idx // n, idx % n
    return dict(w=w, wv=wv, bv=bv, rows=buf["obs"][slot, :, env].T, ts=buf["ts"][slot, env],
                actions=buf["actions"][slot, :, env], old_lp=np.asarray(old_lp)[slot, env],
                adv=buf["adv"][slot, env], ret=buf["ret"][slot, env])
