"""Restatements for the tests of the train sequence (include/oc_policy.h, the last section) -- not a
test module.  Builds on tests/ppo_ref.py, which it leaves as it is.

    perm(seed, epoch, N)                 the epoch permutation, from the header's prose, in numpy
    expand(perm, granule), cuts(...)     idx as oc_policy_ppo_epoch_begin writes it; train()'s minibatches
    vclip_reference(case, old_v, c, ...) the float64 value-clipped loss and gradient with their bounds
    old_values(buf)                      the recorded values of ppo_ref.make_buffer's `old` module
    vclip_inputs()                       the inputs the value-clipping tests share, CPU and GPU
"""
import numpy as np

import policy_ac_ref as ar
import policy_ref as pr
import ppo_ref as pp

U = pp.U
M32 = np.uint64(0xFFFFFFFF)
WALK_CAP = 4096
VCLIP_MUTATIONS = ("ignored", "mask_inverted", "clamp_around_zero", "grad_unclipped")
TRAIN_STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss")


# ---- the permutation ------------------------------------------------------------------------------
def fmix32(h):
    """murmur3's finaliser on uint64 arrays holding 32-bit words."""
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def shuffle_bits(N):
    b = 2
    while (1 << b) < N:
        b += 2
    return b


def perm(seed, epoch, N):
    """(perm int32 [N], the longest walk in passes)."""
    half = np.uint64(shuffle_bits(N) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    keys = [fmix32(np.uint64((seed ^ ((0x9E3779B9 * (4 * epoch + r + 1)) & 0xFFFFFFFF)) & 0xFFFFFFFF)) for r in range(4)]

    def one_pass(x):
        L, R = x >> half, x & mask
        for k in keys:
            L, R = R, L ^ (fmix32(R ^ k) & mask)
        return (L << half) | R

    x = one_pass(np.arange(N, dtype=np.uint64))
    walks = 1
    out = np.asarray(x >= np.uint64(N))
    while out.any():
        assert walks < WALK_CAP
        x[out] = one_pass(x[out])
        out = x >= np.uint64(N)
        walks += 1
    return x.astype(np.int32), walks


def expand(p, granule):
    """idx[i * g + j] = perm[i] * g + j."""
    g = int(granule)
    return (np.asarray(p, np.int64)[:, None] * g + np.arange(g)[None, :]).reshape(-1).astype(np.int32)


def cuts(total, batch_size):
    """train()'s minibatches as (offset, size): batch_size each, the last one shorter, a remainder of
    one sample dropped."""
    bs = int(batch_size or total)
    return [(o, min(bs, total - o)) for o in range(0, total, bs) if min(bs, total - o) >= 2]


# ---- value clipping -------------------------------------------------------------------------------
def old_values(buf):
    """The recorded values [T][n] as the float64 emulation of the `old` module gives them, in float32
    (the GPU tests record score()'s: the same to a few float32 ulps)."""
    w, wv, bv = ar.weights(buf["old"])
    T = buf["obs"].shape[0]
    return np.stack([ar.ref_value(w, wv, bv, buf["obs"][s], buf["ts"][s]) for s in range(T)]).astype(np.float32)


def _value_terms(v, old_v, ret, c, mutate):
    """(v_pred, gate) of the header -- or of a planted mutation -- for the loss, and for the gradient."""
    dv = v - old_v
    vp, gate = old_v + np.clip(dv, -c, c), (dv >= -c) & (dv <= c)
    if mutate == "ignored":
        return (v, np.ones_like(gate)), (v, np.ones_like(gate))
    if mutate == "mask_inverted":
        return (vp, gate), (vp, ~gate)
    if mutate == "clamp_around_zero":
        z = (np.clip(v, -c, c), (v >= -c) & (v <= c))
        return z, z
    if mutate == "grad_unclipped":
        return (vp, gate), (v, np.ones_like(gate))
    return (vp, gate), (vp, gate)


def vclip_reference(case, old_v, c, hp, plan=None, emulate=True, mutate=None):
    """The header's value-clipped loss on the minibatch `case` (ppo_ref.make_case) with the recorded
    values `old_v` [B] and c = clip_range_vf > 0, in float64.

    How: ppo_ref.loss_and_grad's value row is d_i = 2 vf (v_i - ret_i).  The clipped loss has
    d_i = 2 vf (v_pred_i - ret_i) where the gate is open and 0 where it is shut, so it is ppo_ref's
    gradient for the returns ret'_i = v_i - (v_pred_i - ret_i) (open) or v_i (shut): nothing else of
    the loss looks at the returns.  value_loss and loss are then formed here from v_pred.

    Returns (grads, stats, info); with `plan` also the bounds: info["bound"] (unclipped gradient, as
    ppo_ref.grad_bound's), info["stat_bound"], info["margin"] = min_i (| |v_i - old_v_i| - c | - e_i)
    over the good samples, e_i = ppo_ref's bound on the kernel's value plus the roundings of the
    float32 subtraction and comparison, 3 u (|v_i| + |old_v_i| + c): where the margin is positive the
    kernel takes every sample's gate as the reference does, which the bounds below rely on.

    The bounds are ppo_ref.grad_bound's for the returns ret', which charge the value row
    2 vf lb_v + 3 u |d|, plus what the clipped form adds: with the gate open the kernel forms
    old_v + (v - old_v) in float32 instead of v, two roundings, e_x = 2 u (|v| + |old_v|) per sample
    (shut: d is an exact 0 on both sides).  That error of d = 2 vf e_x enters wv, bv and, through
    dh = W2^T d, the first layer, linearly, against h and tanh' at their largest (ppo_ref.grad_bound's
    e_h and e_s on top of the reference's), times 1.001 for the float32 sums over the samples (gamma(K)
    of ppo_ref is below 1e-4 here).  value_loss takes ppo_ref's formula
    with the value's error lb_v replaced by lb_v + e_x (open) or u |v_pred| (shut: old_v +- c, one
    rounding)."""
    old_v, c = np.asarray(old_v, np.float64), float(np.float32(c))
    _, _, it0 = pp.loss_and_grad(case, hp, emulate=emulate)
    v, ret = it0["net"]["value"], np.asarray(case["ret"], np.float64)
    (vp_l, _), (vp_g, gate_g) = _value_terms(v, old_v, ret, c, mutate)
    eff = dict(case, ret=np.where(gate_g, v - (vp_g - ret), v))
    grads, stats, it = pp.loss_and_grad(eff, hp, emulate=emulate)
    good = it["good"].astype(np.float64)
    B = good.shape[0]
    stats = dict(stats)
    stats["value_loss"] = float((((ret - vp_l) ** 2) * good).sum() / B)
    stats["loss"] = stats["policy_loss"] + hp.ent * stats["entropy_loss"] + hp.vf * stats["value_loss"]
    stats["grad_norm"] = float(np.sqrt(sum((g ** 2).sum() for g in grads.values())))
    info = dict(v=v, gate=gate_g, v_pred=vp_l, good=it["good"], eff=eff)
    if plan is None:
        return grads, stats, info
    bound, sb, ref, rstats = pp.grad_bound(eff, hp, plan)
    lb, linfo = pr.logit_bound(*ar.stack(case["w"], case["wv"], case["bv"]), case["rows"], case["ts"])
    lbv, window = lb[-1], linfo["window"]
    e_x = 2 * U * (np.abs(v) + np.abs(old_v))
    e_d = np.where(gate_g, 2 * hp.vf * e_x, 0.0) * good                     # [B], on d = B d loss / d v
    net = it["net"]
    r = net["f"]["r"]
    s = r * (1 - r)
    h_max = np.abs(net["h"]) + 2 * window + U * np.abs(net["h"])            # ppo_ref.grad_bound's e_h
    dact_max = 4 * (s + window * np.abs(1 - 2 * r) + window ** 2 + 2 * U * s)   # and its e_s
    e_dpre = np.abs(net["W2"][-1])[:, None] * e_d[None, :] * dact_max
    e_dW1 = 1.001 * (e_dpre @ np.abs(net["x"]).T) / B
    F = np.asarray(case["w"][0]).shape[1]
    extra = dict(w1=e_dW1[:, :F], wt=e_dW1[:, F], b1=e_dW1[:, F + 1], wv=1.001 * (h_max @ e_d) / B,
                 bv=np.full(1, 1.001 * e_d.sum() / B))
    bound = {k: b + np.asarray(extra[k]).reshape(b.shape) if k in extra else b for k, b in bound.items()}
    e_vp = np.where(gate_g, lbv + e_x, U * np.abs(vp_l))
    G, tpw = int(plan[0]), int(plan[1])
    acc = (tpw + 3) * U
    val_d = np.abs(ret - vp_l)
    sb = dict(sb)
    sb["value_loss"] = float(((2 * val_d * e_vp + e_vp ** 2 + (3 * U + acc) * val_d ** 2) * good).sum() / B)
    sb["loss"] = sb["policy_loss"] + hp.ent * sb["entropy_loss"] + hp.vf * sb["value_loss"] + U * (
        abs(stats["policy_loss"]) + hp.ent * abs(stats["entropy_loss"]) + hp.vf * abs(stats["value_loss"]))
    e2 = float(np.sqrt(sum((b ** 2).sum() for b in bound.values())))
    first = (sum((np.abs(grads[k]) * bound[k]).sum() for k in bound) + 0.5 * e2 * e2) / max(stats["grad_norm"], 1e-300)
    sb["grad_norm"] = min(e2, first) + U * stats["grad_norm"]
    e_i = lbv + 3 * U * (np.abs(v) + np.abs(old_v) + c)
    margin = (np.abs(np.abs(v - old_v) - c) - e_i)[it["good"]]
    info.update(bound=bound, stat_bound=sb, margin=float(margin.min()), marginal=rstats["marginal"])
    return grads, stats, info


# ---- the value-clipping tests' shared inputs ------------------------------------------------------------
VCASE = pp.GRAD_CASES[3]            # F = 46, C = 3, float32 rows, scale 4, B = 210, one workgroup: the GPU test's
VSEED = 3                           # the seed of the GPU test's device shuffle
_cache = {}


def vclip_inputs():
    """The GPU test's inputs (tests/test_ppo_train_gpu.py takes them from here): the whole 210-sample buffer
    as one minibatch in the order of the device permutation, and clip_range_vf = the median of the
    reference's |v - old_v|, so that half of the samples fall on each side."""
    if "v" not in _cache:
        F, C, odt, scale, B, mg, seed = VCASE
        buf = pp.make_buffer(F, C, odt, scale, seed)
        idx = expand(perm(VSEED, 0, B)[0], 1)
        case = pp.make_case(buf, idx, pp.old_log_probs(buf))
        old_v = old_values(buf).reshape(-1)[idx]
        _, _, it = pp.loss_and_grad(case, pp.test_hp())
        c = float(np.float32(np.median(np.abs(it["net"]["value"] - old_v.astype(np.float64)))))
        _cache["v"] = dict(buf=buf, idx=idx, case=case, old_v=old_v, c=c, plan=pp.ref_plan(B, mg), mg=mg)
    return _cache["v"]
