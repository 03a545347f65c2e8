"""Restatements for the tests of the recurrent learner's train sequence (include/oc_policy.h, last section:
oc_policy_recurrent_train_step) -- not a test module.  Builds on tests/recurrent_ppo_ref.py (the float64 loss and
its gradient through time) and tests/ppo_train_ref.py (the permutation), which it leaves as they are.

    recorded_values(case)                       the values a rollout would have recorded, float32 [T][n]
    clipped_loss_and_grad(case, old_v, c, ...)  the value-clipped loss and its gradient, float64
    gate_conditions(case, old_v, c)             (share of open gates, min | |v - old_v| - c |)
    epoch_envs(seed, epoch, n, granule)         idx as oc_policy_ppo_epoch_begin writes it for count = n
    vclip_moves(case, old_v, c, hp)             how far each planted value-clipping bug moves the gradient

The gradient identity.  The gradient through time is linear in D = d (B loss) / d [logits; value], and the value
head's row is 2 vf (v_pred - ret) where the gate is open -- where v_pred = v -- and 0 where it is shut.  So the
clipped gradient is recurrent_ppo_ref.loss_and_grad's for the returns ret' = ret (open) or v, the forward's own
value (shut: the row is 2 vf (v - v), an exact 0); nothing else of the gradient looks at the returns.  value_loss
and loss are formed here, from the clamp directly.

Tolerances: recurrent_ppo_ref's TOL_G and TOL_S -- the clipped gradient is the same arithmetic with some value
terms zeroed.  MEASURED below is what tests/test_recurrent_train_gpu.py printed on an MI355X.
"""
import numpy as np

import ppo_train_ref as tr
import recurrent_ppo_ref as rp

C_VF = 0.1                          # clip_range_vf of the value-clipping tests
VCLIP_MUTANTS = ("clipping ignored", "gradient not gated", "clamped about the return")

# ---- measured on an MI355X, 2026-10-21, tests/test_recurrent_train_gpu.py, case c with every env in one minibatch,
# clip_range_vf 0.1, max_groups 0 and 1: the largest ``rel_diff`` over the eight tensors and the largest
# ``stats_diff`` over the ten statistics against clipped_loss_and_grad(emulate=True).  Both within
# recurrent_ppo_ref's TOL_G = 2.8e-4 and TOL_S = 2.2e-6, which therefore stand as they are.
MEASURED = dict(grad=dict(c=1.03e-05, c_one_group=1.03e-05), stats=dict(c=1.61e-06, c_one_group=1.61e-06))
# (the largest gradient figure is w2's, the largest statistic grad_norm's; value_loss 6.9e-08.  Against the
# UNCLIPPED reference the same kernel output lies 0.0104 off in value_loss and 0.61 off in the gradient.)


def all_envs(case):
    """The case with every env of its sink once as the minibatch."""
    return dict(case, envs=np.arange(case["n"], dtype=np.int32))


def recorded_values(case, seed=0):
    """float32 [T][n]: the emulated current value of every sample moved by +-0.02 or +-0.3, times U(0.9, 1.1) --
    recurrent_ppo_ref.make_case's scheme for the recorded log-probs: with clip_range_vf = 0.1 about half of the
    gates are open, and no sample sits near the edge of the clamp, where the gradient is discontinuous."""
    rng = np.random.default_rng(8100 + seed)
    T, n = case["T"], case["n"]
    v = rp.loss_and_grad(all_envs(case), rp.test_hp())[2]["value"]             # [T][n]
    delta = rng.choice([-0.3, -0.02, 0.02, 0.3], (T, n)) * rng.uniform(0.9, 1.1, (T, n))
    return (v + delta).astype(np.float32)


def _terms(v, old, ret, c, mutate):
    """((v_pred, gate) of the loss, (v_pred, gate) of the gradient) -- the header's, or a planted bug's."""
    dv = v - old
    vp, gate = old + np.clip(dv, -c, c), (dv >= -c) & (dv <= c)
    everywhere = np.ones_like(gate)
    if mutate == "clipping ignored":
        return (v, everywhere), (v, everywhere)
    if mutate == "gradient not gated":
        return (vp, gate), (vp, everywhere)
    if mutate == "clamped about the return":
        z = (ret + np.clip(v - ret, -c, c), (v - ret >= -c) & (v - ret <= c))
        return z, z
    if mutate is not None:
        raise ValueError("unknown mutant %r" % (mutate,))
    return (vp, gate), (vp, gate)


def clipped_loss_and_grad(case, old_v, c, hp, emulate=True, mutate=None):
    """The header's value-clipped loss over the minibatch of ``case`` with the recorded values ``old_v``
    (float32 [T][n]) and c = clip_range_vf > 0, in float64: (grads, stats, info) as recurrent_ppo_ref.loss_and_grad's,
    info with ``gate`` [T][E], ``v``, ``v_pred``."""
    envs = np.asarray(case["envs"], np.int64)
    c = float(np.float32(c))
    _, _, it0 = rp.loss_and_grad(case, hp, emulate=emulate)
    v = it0["value"]                                                           # [T][E]
    old = np.asarray(old_v, np.float64)[:, envs]
    ret = np.asarray(case["ret"], np.float64)[:, envs]
    (vp_l, _), (vp_g, gate_g) = _terms(v, old, ret, c, mutate)
    # D's value row becomes 2 vf (v - ret') = 2 vf (v_pred - ret) where the gate is open, 0 where it is shut; a
    # repeated env brings the same sequence twice, so its two writes agree
    eff = np.asarray(case["ret"], np.float64).copy()
    eff[:, envs] = np.where(gate_g, v - (vp_g - ret), v)
    grads, stats, it = rp.loss_and_grad(dict(case, ret=eff), hp, emulate=emulate)
    good = it["good"].astype(np.float64)
    B = good.shape[0]
    stats = dict(stats)
    stats["value_loss"] = float((((ret - vp_l).reshape(-1) ** 2) * good).sum() / B)
    stats["loss"] = stats["policy_loss"] + hp.ent * stats["entropy_loss"] + hp.vf * stats["value_loss"]
    return grads, stats, dict(it, gate=gate_g, v=v, v_pred=vp_l)


def gate_conditions(case, old_v, c):
    """(the share of open gates, min | |v - old_v| - c |) over the minibatch, from the emulated forward."""
    envs = np.asarray(case["envs"], np.int64)
    v = rp.loss_and_grad(case, rp.test_hp())[2]["value"]
    dv = np.abs(v - np.asarray(old_v, np.float64)[:, envs])
    c = float(np.float32(c))
    return float((dv <= c).mean()), float(np.abs(dv - c).min())


def vclip_moves(case, old_v, c, hp):
    """{mutant: the largest relative move (``rel_diff``) it causes in any tensor of the emulated gradient}."""
    ref = clipped_loss_and_grad(case, old_v, c, hp)[0]
    return {m: max(rp.rel_diff(clipped_loss_and_grad(case, old_v, c, hp, mutate=m)[0], ref).values())
            for m in VCLIP_MUTANTS}


def epoch_envs(seed, epoch, n, granule):
    """int32 [n]: the permutation of the envs oc_policy_ppo_epoch_begin(count = n, granule, seed) writes in the
    epoch numbered ``epoch``."""
    return tr.expand(tr.perm(seed, epoch, n // granule)[0], granule)


def env_cuts(n, T, envs_per_batch):
    """The recurrent train()'s minibatches as (offset, E): chunks of ``envs_per_batch`` envs in order, a last chunk
    with E T < 2 dropped -- ``RecurrentPPOLearner.minibatches``' sizes, restated."""
    per = int(envs_per_batch or n)
    return [(o, min(per, n - o)) for o in range(0, n, per) if min(per, n - o) * T >= 2]
