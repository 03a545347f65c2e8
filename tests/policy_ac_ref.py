"""A float64 restatement of the actor-critic form of the fused MLP policy (include/oc_policy.h:
oc_policy_mlp_ac) for the tests -- not a test module.  It builds on tests/policy_ref.py and, like
it, is written from the module's plain weights and the header's definitions, never from the packed
fragments.

The value head is one more row of the second product, folded exactly as a logit row is, so it IS
``policy_ref._forward`` with ``[w2; wv]`` as the row matrix and ``[b2; bv]`` as the bias: the last row.

    ref_value(w, wv, bv, rows, ts, emulate)        the value [n]
    value_bound(w, wv, bv, rows, ts)               policy_ref.logit_bound of that row
    ref_log_prob(w, rows, ts, actions, emulate)    (log_prob [n], per-head terms [2][n])
    log_prob_bound(w, rows, ts, actions)           how far the kernel's log_prob may lie from it

``w`` is the tuple (w1, wt, b1, w2, b2) of float64 arrays policy_ref takes.
"""
import numpy as np

import policy_ref as pr

U = pr.U_F32          # 2^-23: one fp32 ulp, the unit roundoff charged for every fp32 operation
HEADS = ((0, 4), (4, None))       # logit rows of the move head and of the comm head (to 4 + C)


def stack(w, wv, bv):
    """The weights with the value head as one more row of the second layer."""
    w1, wt, b1, w2, b2 = w
    return (w1, wt, b1, np.concatenate([np.asarray(w2, np.float64), np.asarray(wv, np.float64).reshape(1, -1)]),
            np.concatenate([np.asarray(b2, np.float64).reshape(-1), np.asarray(bv, np.float64).reshape(-1)]))


def ref_value(w, wv, bv, rows, ts, emulate=True, fold=True):
    return pr.ref_logits(*stack(w, wv, bv), rows, ts, emulate=emulate, fold=fold)[-1]


def value_bound(w, wv, bv, rows, ts):
    """|kernel value - ref_value(emulate=True)| <= this, [n]: the bound is per row."""
    return pr.logit_bound(*stack(w, wv, bv), rows, ts)[0][-1]


def head_log_softmax(logits):
    """ln softmax over axis 0 in float64, [K][n]."""
    x = np.asarray(logits, np.float64)
    m = x.max(axis=0, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=0, keepdims=True))


def _gather(ls, a):
    """ls[a[i]][i], -inf where a[i] is outside 0..K-1."""
    K, n = ls.shape
    ok = (a >= 0) & (a < K)
    out = np.full(n, -np.inf)
    out[ok] = ls[a[ok], np.arange(n)[ok]]
    return out


def ref_log_prob(w, rows, ts, actions, emulate=True):
    """actions int [n][2] = (move, comm).  Returns (lp_move + lp_comm [n], the two terms [2][n])."""
    logits = pr.ref_logits(*w, rows, ts, emulate=emulate)
    actions = np.asarray(actions).astype(np.int64)
    terms = np.stack([_gather(head_log_softmax(logits[lo:hi]), actions[:, col])
                      for col, (lo, hi) in enumerate(HEADS)])
    return terms[0] + terms[1], terms


def log_prob_bound(w, rows, ts, actions):
    """Bound [n] on |kernel log_prob - ref_log_prob(emulate=True)| for in-range actions:

        sum over the two heads of (bound_a + max_c bound_c)  +  arith

    The first part is what the logits' own error (policy_ref.logit_bound, per row) can do:
    ln softmax(L)[a] = L_a - logsumexp(L), and logsumexp moves by at most max_c |dL_c| when every
    L_c moves by dL_c (its gradient is a probability vector).

    ``arith`` bounds the kernel's own float32 chain behind its logits, per head, with base-2 logits
    L_c, count candidates, u = 2^-23 per operation (one full ulp, as in policy_ref):

        d_c = L_c - m                   one subtraction:            |err| <= u |d_c|    (d_m = 0 exactly)
        e_c = v_exp_f32(d_c)            1 ulp, and the error of d_c passes through 2^x:
                                        |err| <= u e_c + ln 2 u |d_c| 2^d_c <= u e_c + 0.37 u
                                        (x 2^-x <= 1 / (e ln 2) = 0.531; ln 2 * 0.531 < 0.37);
                                        results below 2^-126 may be flushed: 2^-126 each
        S = sum e_c                     count - 1 additions (the padding terms are exact zeros):
                                        |err| <= gamma(count - 1) S + sum of the e_c errors, and S >= 1
                                        (the maximum contributes 2^0), so relative to S
                                        rel_S <= gamma(count - 1) + u + count (0.37 u + 2^-126)
        g = v_log_f32(S)                1 ulp of the result, charged as u max(|log2 S|, 1), and
                                        rel_S passes through as rel_S / ln 2 (base 2), inflated by
                                        1 / (1 - rel_S)
        q = d_a - g                     u |q|
        lp = q * K_LN2                  the float K_LN2 is itself rounded: 2 u |lp| (policy_ref)
      log_prob = lp_move + lp_comm      u |log_prob|

    The magnitudes |d_a|, |log2 S|, |q|, |lp| are taken from the emulated reference and enlarged by
    the head's logit part of the bound, so that they cover the kernel's own values.  For C = 1 the
    comm head is exact (d = 0, S = 1, log2 1 = 0) and its terms vanish up to the 1-ulp floor."""
    logits = pr.ref_logits(*w, rows, ts)
    lb, _ = pr.logit_bound(*w, rows, ts)
    actions = np.asarray(actions).astype(np.int64)
    n = logits.shape[1]
    total = np.zeros(n)
    lps = np.zeros(n)
    for col, (lo, hi) in enumerate(HEADS):
        L, b = logits[lo:hi] / pr.LN2, lb[lo:hi]              # base 2
        count = L.shape[0]
        a = np.clip(actions[:, col], 0, count - 1)
        part = b[a, np.arange(n)] + b.max(axis=0)             # natural log
        slack = part / pr.LN2
        m = L.max(axis=0)
        d_a = np.abs(L[a, np.arange(n)] - m) + slack
        S = np.exp2(L - m).sum(axis=0)
        g = np.abs(np.log2(S)) + slack
        rel_S = pr._gamma(count - 1) + U + count * (0.37 * U + 2.0 ** -126)
        q = d_a + g
        base2 = U * d_a + U * np.maximum(g, 1.0) + rel_S / (pr.LN2 * (1 - rel_S)) + U * q
        lp = q * pr.LN2
        total += part + pr.LN2 * base2 + 2 * U * lp
        lps += lp
    return total + U * lps


def make_actor_critic(F, C, seed, scale):
    """``MLPActorCritic(seed)`` (CPU) with its first layer re-drawn for F features (same init rule)
    and every weight scaled by `scale`: tests/test_policy_reference_gpu.py's ``_policy`` with the
    value head."""
    import torch
    from gym_comm_amd.vec_env import MLPActorCritic
    pol = MLPActorCritic(3, C, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        pol.w1 = torch.nn.Parameter((torch.rand((64, F), generator=g) * 2 - 1) / float(np.sqrt(F)))
        for t in (pol.w1, pol.b1, pol.wt, pol.w2, pol.b2, pol.wv, pol.bv):
            t.mul_(scale)
    return pol


def weights(pol):
    """((w1, wt, b1, w2, b2), wv, bv) of a module as float64 arrays."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)
    return tuple(f(t) for t in (pol.w1, pol.wt, pol.b1, pol.w2, pol.b2)), f(pol.wv), f(pol.bv)


def make_rows(F, n, odt, seed):
    """tests/test_policy_reference_gpu.py's ``_rows`` as a numpy array: mostly small values, one
    element in ten from the type's whole range, both ends present."""
    rng = np.random.default_rng(seed)
    if odt == "float32":
        small, big, lo, hi = rng.uniform(-2, 2, (F, n)), rng.uniform(-2048, 2048, (F, n)), -2047.7, 2047.3
    else:
        lo, hi = (-128, 127) if odt == "int8" else (-2048, 2048)
        small, big = rng.integers(-2, 3, (F, n)), rng.integers(lo, hi + 1, (F, n))
    x = np.where(rng.random((F, n)) < 0.1, big, small)
    x.flat[0] = lo
    x.flat[-1] = hi
    return x.astype({"int32": np.int32, "int8": np.int8, "float32": np.float32}[odt])


def make_timesteps(n, T, seed):
    return np.random.default_rng(seed + 7).integers(0, T + 1, n) / float(T)
