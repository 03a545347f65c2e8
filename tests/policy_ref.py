"""A float64 restatement of the fused MLP policy (include/oc_policy.h, csrc/oc_policy_device.h) for
the tests -- not a test module.

It is written from the module's plain weights (vec_env.MLPPolicy: w1 [64][F], wt [64], b1 [64],
w2 [4 + C][64], b2 [4 + C]) and the header's definitions, not from the packed fragments, so it
shares no code with the packer (the CPU tests check that the two agree on every rounding).

    ref_logits(..., emulate=False)   the exact module, W2 tanh(W1 x + wt ts + b1) + b2
    ref_logits(..., emulate=True)    the same with exactly the roundings the header defines, and
                                     nothing else (see ``_forward``)
    logit_bound(...)                 how far the kernel's logits may lie from the emulated ones
    pcg32 / draw_u / ref_sample      the sampler: PCG32 -> uniform -> inverse CDF, in fp64
"""
import numpy as np

LOG2E32 = np.float32(1.4426950408889634)      # ocpol::K_LOG2E, the constant the packer folds in
LN2 = float(np.log(2.0))
HIDDEN = 64
PCG_MULT, PCG_INC, PCG_OUT_MULT = 747796405, 2891336453, 277803737   # oc_policy_device.h: pcg32
U32 = np.uint64(0xFFFFFFFF)

# unit roundoff used for every fp32 operation of the kernel: 2^-23, one full fp32 ulp, so that the
# bound holds whatever rounding (nearest or toward zero) the matrix cores use inside an MFMA
U_F32 = 2.0 ** -23
# relative error of r = v_rcp_f32(v_exp_f32(a) + 1) against 1 / (2^a + 1) at the kernel's a:
# v_exp_f32 1 ulp, the add half an ulp, v_rcp_f32 1 ulp -- 2.5 ulp, taken as 4
EPS_R = 4 * U_F32


def comm_row(c):
    """Row of the second product that holds comm logit c (oc_policy.h)."""
    return 4 + (c & 3) + 8 * (c >> 2)


def _f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def fold_w1(w1, wt, b1):
    """The fp16 values the first product multiplies by: 2 log2(e) [W1 | wt | b1], the product
    taken in fp32 (as the packer does) and rounded to fp16.  float64 [64][F + 2]."""
    w1 = np.asarray(w1, np.float32)
    aug = np.concatenate([w1, np.asarray(wt, np.float32).reshape(-1, 1),
                          np.asarray(b1, np.float32).reshape(-1, 1)], axis=1)
    return _f16((np.float32(2) * LOG2E32) * aug)


def fold_w2(w2):
    """W2' = -2 log2(e) W2 (fp32 product, rounded to fp16).  float64 [4 + C][64]."""
    return _f16((np.float32(-2) * LOG2E32) * np.asarray(w2, np.float32))


def fold_b2(b2, w2):
    """b2' = log2(e) b2 - 1/2 sum_j W2'[.][j] over the ROUNDED W2', in fp32 with the packer's
    order (j = 0..63 in sequence).  float64 [4 + C]."""
    w2h = fold_w2(w2).astype(np.float32)
    s = np.zeros(w2h.shape[0], np.float32)
    for j in range(w2h.shape[1]):
        s = (s + w2h[:, j]).astype(np.float32)
    lb = (LOG2E32 * np.asarray(b2, np.float32).reshape(-1)).astype(np.float32)
    return (lb - np.float32(0.5) * s).astype(np.float32).astype(np.float64)


def features(rows, ts):
    """The first product's B operand as the kernel forms it: the rows converted to float32 and
    then fp16, the timestep double -> float32 -> fp16, the constant 1.  float64 [F + 2][n]."""
    x = _f16(np.asarray(rows).astype(np.float32))
    t = _f16(np.asarray(ts, np.float64).astype(np.float32)).reshape(1, -1)
    return np.concatenate([x, t, np.ones_like(t)], axis=0)


def _forward(w1, wt, b1, w2, b2, rows, ts, act="tanh", fold=True):
    """The emulated network.  Beyond fp64, exactly the roundings oc_policy.h defines:
    features / timestep / 1 and 2 log2(e) [W1 | wt | b1] and -2 log2(e) W2 in fp16, b2' in fp32
    (the packer's), r = 1 / (2^a + 1) exact then rounded to fp16.  Returns a dict of the
    intermediates (base-2 logits ``L2`` in the module's row order [4 + C][n]).
    ``act`` / ``fold`` exist for the tests' planted mutations only: act="r" feeds r where the
    network has tanh (W2 r + b2), fold=False drops the row-sum fold from b2'."""
    A = fold_w1(w1, wt, b1)                              # [64][F + 2]
    X = features(rows, ts)                               # [F + 2][n]
    a = A @ X                                            # fp16 x fp16 products: exact in fp64
    with np.errstate(over="ignore"):
        r = 1.0 / (np.exp2(a) + 1.0)
    rh = _f16(r)
    W2h = fold_w2(w2)
    b2p = fold_b2(b2, w2)
    if act == "r":
        L2 = LOG2E32 * (np.asarray(w2, np.float64) @ rh + np.asarray(b2, np.float64).reshape(-1, 1))
    else:
        L2 = W2h @ rh + b2p.reshape(-1, 1)
        if not fold:
            L2 = L2 + 0.5 * W2h.sum(axis=1, keepdims=True)
    return dict(A=A, X=X, a=a, r=r, rh=rh, W2h=W2h, b2p=b2p, L2=L2)


def ref_logits(w1, wt, b1, w2, b2, rows, ts, emulate=True, act="tanh", fold=True):
    """Natural-log logits [4 + C][n] in float64 (rows 0..3 move, 4 + c comm c).
    emulate=False: the exact module; emulate=True: with the header's roundings (``_forward``)."""
    if emulate:
        return _forward(w1, wt, b1, w2, b2, rows, ts, act, fold)["L2"] * LN2
    x = np.asarray(rows).astype(np.float64)
    t = np.asarray(ts, np.float64).reshape(1, -1)
    h = (np.asarray(w1, np.float64) @ x + np.asarray(wt, np.float64).reshape(-1, 1) * t
         + np.asarray(b1, np.float64).reshape(-1, 1))
    hid = np.tanh(h) if act == "tanh" else 1.0 / (np.exp(2 * h) + 1.0)
    return np.asarray(w2, np.float64) @ hid + np.asarray(b2, np.float64).reshape(-1, 1)


def _gamma(k):
    return k * U_F32 / (1 - k * U_F32)


def logit_bound(w1, wt, b1, w2, b2, rows, ts):
    """Per-element bound [4 + C][n] on |kernel logit - ref_logits(emulate=True)| (natural log).

    After emulation the kernel differs from the reference in three ways only:

    1. fp32 accumulation inside the MFMA.  The products of two fp16 values are exact in fp32; a
       sum of K terms accumulated in any order with a rounding of at most u = 2^-23 per addition is
       off by at most gamma(K) = K u / (1 - K u) times the sum of the terms' magnitudes.  First
       product: K = 16 ksteps + 1 terms, so  |a_kernel - a| <= da = gamma(K) sum_k |A_k X_k|.
       Second product: 64 terms + the start value b2', so it adds
       gamma(66) (|b2'| + sum_j |W2'_j| (r16_j + ulp16(r16_j))).
    2. v_exp_f32 / v_add / v_rcp_f32.  The kernel's r before its fp16 rounding is
       1 / (2^a_kernel + 1) (1 + d), |d| <= EPS_R = 4 u, and 1 / (2^a + 1) moves by at most
       ln 2 rr da with a moving by da, rr = max r (1 - r) over [a - da, a + da]
       (<= r (1 - r) 2^da, and <= 1/4).  So the kernel's unrounded r lies within the window
       w_j = ln 2 rr da + EPS_R r of the exact one.
    3. The fp16 rounding of r then lands on the same fp16 value as the reference's, except when
       the exact r lies within w_j of a rounding midpoint (the window, relative to r, is stated
       above: a few fp32 ulps of r plus the first product's share).  Only such hidden units are
       charged, one fp16 ulp of r (the larger neighbour gap) times |W2'_oj| each -- NOT every
       unit a full fp16 ulp (that worst case would be ~1e-2).

    The sum is in base 2; it is converted with ln 2 and the kernel's fp32 product
    ``out * K_LN2`` (the float K_LN2 is itself rounded) adds 2^-22 |logit|."""
    f = _forward(w1, wt, b1, w2, b2, rows, ts)
    F = np.asarray(w1).shape[1]
    ksteps = (F + 2 + 15) // 16
    da = _gamma(16 * ksteps + 1) * (np.abs(f["A"]) @ np.abs(f["X"]))          # [64][n]
    r = f["r"]
    rr = np.minimum(0.25, r * (1.0 - r) * np.exp2(da))
    window = LN2 * rr * da + EPS_R * r
    rh16 = f["rh"].astype(np.float16)
    lo = np.nextafter(rh16, np.float16(-np.inf)).astype(np.float64)
    hi = np.nextafter(rh16, np.float16(np.inf)).astype(np.float64)
    rh = f["rh"]
    dist = np.minimum(np.abs(r - 0.5 * (lo + rh)), np.abs(r - 0.5 * (rh + hi)))
    ulp = np.maximum(rh - lo, hi - rh)
    flip = (dist <= window).astype(np.float64)
    W2a = np.abs(f["W2h"])
    b2 = W2a @ (flip * ulp)
    b2 += _gamma(66) * (np.abs(f["b2p"]).reshape(-1, 1) + W2a @ (rh + ulp))
    return LN2 * b2 + 2.0 ** -22 * np.abs(f["L2"] * LN2), dict(flipped=flip, window=window)


def pcg32(state):
    """The kernel's generator (oc_policy_device.h: pcg32), vectorised over uint32 states held in
    any integer array (int32 bit patterns included).  Returns (new state, output), both uint64
    arrays of values < 2^32."""
    s = np.asarray(state).astype(np.int64).astype(np.uint64) & U32
    s = (s * np.uint64(PCG_MULT) + np.uint64(PCG_INC)) & U32
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(PCG_OUT_MULT)) & U32
    return s, (w >> np.uint64(22)) ^ w


def draw_u(out):
    """The uniform draw of one PCG32 output: u = ((x >> 8) + 1/2) / 2^24, in (0, 1), exactly as
    oc_policy.h defines it.  (The kernel forms it in fp32, where (x >> 8) + 0.5 rounds for
    x >> 8 >= 2^23: its u is off by at most 2^-25 -- inside every margin the tests use.)"""
    return ((np.asarray(out, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0


def ref_sample(base2_logits, u):
    """Inverse CDF of the softmax of base-2 logits [K][n] with the uniform draws u [n], in fp64:
    the action is the number of cumulative sums (of the first K - 1 probabilities) that do not
    exceed u * total.  Returns (action int64 [n], margin [n]): the distance from u * total to the
    nearest cumulative boundary, relative to the total (inf for K = 1)."""
    x = np.asarray(base2_logits, np.float64)
    p = np.exp2(x - x.max(axis=0, keepdims=True))
    total = p.sum(axis=0)
    t = np.asarray(u, np.float64) * total
    cum = np.cumsum(p, axis=0)[:-1]
    action = (cum <= t).sum(axis=0).astype(np.int64)
    if cum.shape[0] == 0:
        return action, np.full(x.shape[1], np.inf)
    return action, (np.abs(cum - t) / total).min(axis=0)


def first_argmax(logits):
    """torch.argmax's rule on these sizes: the first maximum."""
    return np.asarray(logits).argmax(axis=0)
