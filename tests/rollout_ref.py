"""Reference for the rollout buffer's returns and advantages (include/oc_rollout.h): numpy only, no
code shared with the product.

stable-baselines3's ``RolloutBuffer.compute_returns_and_advantage`` over CHRONOLOGICAL arrays
(row 0 = oldest step), per env, newest to oldest:

    nnt   = 1 - (k == L-1 ? last_dones : episode_starts[k+1])
    nv    =      k == L-1 ? last_values : values[k+1]
    delta = (rewards[k] + (g * nv) * nnt) - values[k]
    last  = delta + ((gl * nnt) * last)
    advantages[k] = last;  returns[k] = last + values[k]

``gae(..., dtype=np.float32)`` rounds every operation to float32 in exactly that order (rewards
are rounded to float32 first, g = float32(gamma), gl = float32(gamma * gae_lambda) with the product
in double); ``dtype=np.float64`` is the same loop without any rounding to float32.

``add_plan(n, F)`` restates how ``oc_rollout_add`` shapes its launch (csrc/oc_rollout.hip), from that
file's description of it, for the CPU tests of ``oc_rollout_add_plan``.
"""
import numpy as np


def gae(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda, dtype=np.float32, gl=None):
    """rewards, values, episode_starts: [L][n]; last_values, last_dones: [n].  Returns
    (advantages, returns), [L][n] of ``dtype``.  ``gl`` replaces the discount of ``last`` (a test's
    planted mutant: the product formed some other way)."""
    dt = np.dtype(dtype).type
    r = np.asarray(rewards, dtype=np.float64).astype(dt)
    v = np.asarray(values).astype(dt)
    es = np.asarray(episode_starts).astype(dt)
    L = r.shape[0]
    g = dt(np.float64(gamma))
    gl = dt(np.float64(gamma) * np.float64(gae_lambda)) if gl is None else dt(gl)
    one = dt(1)
    adv, ret = np.zeros_like(v), np.zeros_like(v)
    nv = np.asarray(last_values).astype(dt)
    nnt = one - np.asarray(last_dones).astype(dt)
    last = np.zeros(v.shape[1:], dtype=dt)
    for k in range(L - 1, -1, -1):
        delta = (r[k] + (g * nv) * nnt) - v[k]
        last = delta + ((gl * nnt) * last)
        assert delta.dtype == dt and last.dtype == dt
        adv[k] = last
        ret[k] = last + v[k]
        nv, nnt = v[k], one - es[k]
    return adv, ret


def add_plan(n, F, target=512, block=256):
    """(gridDim.x, groups, per_group) of ``oc_rollout_add``: a slot is F + 7 row tasks; with
    ``ceil(n / 256)`` blocks of envs, enough groups of tasks to bring the launch to about ``target``
    workgroups, each group the same whole number of consecutive tasks, no group empty; then as many
    columns of env blocks as keep columns x groups within ``target`` -- at least one, never more
    than there are env blocks (a column strides over the rest)."""
    tasks = int(F) + 7
    env_blocks = -(-int(n) // block)
    wanted = min(max(-(-target // env_blocks), 1), tasks)
    per_group = -(-tasks // wanted)
    groups = -(-tasks // per_group)
    columns = min(max(target // groups, 1), env_blocks)
    return columns, groups, per_group


def gl_float32_product(gamma, gae_lambda):
    """The mutant's discount: gamma and lambda rounded to float32 FIRST, then multiplied in float32.
    (0.99, 0.95) cannot tell it from float32(gamma * lambda in double); (0.9, 0.8) and (0.995, 0.97) do."""
    return np.float32(gamma) * np.float32(gae_lambda)


def slots(pos, count, T):
    """Slot of chronological step k = 0 .. L-1, L = min(count, T), in a ring of T slots whose next
    write goes to ``pos``."""
    L = min(int(count), int(T))
    return [(int(pos) - L + k) % int(T) for k in range(L)]


def closed_form(rewards, values, episode_starts, last_values, last_dones):
    """gamma = lambda = 1: the advantage of step k is the sum of the rewards up to the end of its
    episode or of the buffer, plus the bootstrap value where the episode did not end, minus
    values[k]; the return is that plus values[k].  Plain Python integers / floats, per env."""
    r, v, es = np.asarray(rewards), np.asarray(values), np.asarray(episode_starts)
    L, n = v.shape
    adv, ret = np.zeros((L, n)), np.zeros((L, n))
    for i in range(n):
        for k in range(L):
            total, j = 0.0, k
            while True:
                total += float(r[j, i])
                ended = float(last_dones[i]) if j == L - 1 else float(es[j + 1, i])
                if ended:
                    break
                if j == L - 1:
                    total += float(last_values[i])
                    break
                j += 1
            adv[k, i] = total - float(v[k, i])
            ret[k, i] = total
    return adv, ret


def integer_case():
    """T = 6, n = 5, small integers: every float32 operation of the loop is exact at gamma =
    lambda = 1.  Episode starts at the buffer's first step (env 0), its last step (env 1), in the
    middle (env 2), at both ends and twice in a row (env 3), nowhere (env 4); last_dones both ways."""
    rewards = np.array([[1, 0, 2, -1, 3], [0, 2, -2, 1, 0], [3, 1, 0, 0, -1],
                        [-1, 0, 1, 2, 2], [2, -3, 0, 1, 0], [0, 1, 4, -2, 1]], dtype=np.float64)
    values = np.array([[2, -1, 0, 3, 1], [1, 0, -2, 2, 0], [0, 4, 1, -1, 2],
                       [-3, 2, 0, 1, 1], [1, 1, 3, 0, -2], [2, 0, -1, 2, 3]], dtype=np.float32)
    es = np.array([[1, 0, 0, 1, 0], [0, 0, 0, 0, 0], [0, 0, 1, 1, 0],
                   [0, 0, 0, 1, 0], [0, 0, 0, 0, 0], [0, 1, 0, 1, 0]], dtype=np.float32)
    last_values = np.array([5, -2, 3, 1, -4], dtype=np.float32)
    last_dones = np.array([0, 1, 0, 1, 0], dtype=np.float32)
    return rewards, values, es, last_values, last_dones
