"""Adam's lazy replay in float64: the dense reference, a restatement of the kernels' route logic, and the seeded rows.

Both training paths emulate a dense torch.optim.Adam lazily: a row untouched for k steps gets k zero-gradient steps
replayed when it is next read or written.  `opt_replay_row` (bpr_opt.h, STRICT) and `vo_replay` (bpr_vstream.h, the
batched stream) each choose between a closed form (a geometric series with an expansion in eps / sqrt v) and a
per-step loop, by the same three conditions with different constants.  This module states that choice in numpy, so
that tests/test_adam_replay_cpu.py can show on the CPU that the rows the GPU tests seed tell a right replay from a
subtly wrong one, and tests/test_gpu_adam_replay.py can assert which route every seeded row takes before anything is
launched.  No torch, no GPU.
"""
import math

import numpy as np

# per path: series terms, divisor of the sqrt(v) gate, shortest gap that takes the closed form (a function of kmax)
PATHS = {
    "strict": dict(J=12, gate_div=0.2, closed_min=lambda kmax: 16),
    "batched": dict(J=3, gate_div=0.02, closed_min=lambda kmax: 16 if kmax >= 64 else 3),
}
MUTATIONS = ("drop_last_term", "series_k_for_kk", "series_kmax_for_k", "no_gate", "no_closed_min", "no_t_sat",
             "state_kk_for_k")
ZERO_M, TYPICAL, GATE, MIXED, PADDED = range(5)
CLASS_NAMES = ("zero_m", "typical", "gate", "mixed", "padded")
GATE_FACTORS = (0.1, 0.5, 0.9, 1.1, 2.0)  # sqrt(v) / sv_min of the gate rows, for each path's sv_min


def f32(x):
    return float(np.float32(x))


def host_consts(b1, b2):
    """(kmax, t_sat) as opt_dev (bprcore.hip) and vopt (bpr_vstream.hip) compute them from the fp32 betas."""
    b1, b2 = f32(b1), f32(b2)
    kmax = int(math.ceil(math.log(1e-8) / math.log(b1 / math.sqrt(b2))))
    lim = math.log(2.0 ** -25)  # 1 - beta^t rounds to 1.0f once beta^t < 2^-25
    t_sat = int(max(math.ceil(lim / math.log(b1)), math.ceil(lim / math.log(b2))))
    return kmax, t_sat


def sv_min(path, b1, b2, eps):
    """The smallest sqrt(v) that takes the closed form, as the host rounds it to fp32."""
    kmax, _ = host_consts(b1, b2)
    return f32(f32(eps) * f32(b2) ** (-0.5 * kmax) / PATHS[path]["gate_div"])


def path_kw(path, b1, b2):
    kmax, _ = host_consts(b1, b2)
    p = PATHS[path]
    return dict(J=p["J"], gate_div=p["gate_div"], closed_min=p["closed_min"](kmax))


def lane_geometry(d):
    """(G, E) of bpr_bind_tables: element f of a row sits in slot f // G of lane f % G."""
    G = 32 if d <= 128 else 64
    per_lane = -(-d // G)
    E = (1 if per_lane <= 1 else 2 if per_lane <= 2 else 4) if G == 32 else (4 if per_lane <= 4 else 8 if per_lane <= 8 else 16)
    return G, E


def dense_zero_steps(w, m, v, s0, k, lr, b1, b2, eps):
    """Exact float64 dense Adam: the k zero-gradient steps s0+1 ... s0+k.  Returns (w, m, v)."""
    w, m, v = (np.array(a, np.float64) for a in (w, m, v))
    b1, b2, lr, eps = f32(b1), f32(b2), f32(lr), f32(eps)
    for s in range(s0 + 1, s0 + k + 1):
        m *= b1
        v *= b2
        w -= lr / (1.0 - b1 ** s) * (m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** s) + eps))
    return w, m, v


def closed_model(w, m, v, s0, k, lr, b1, b2, eps, J, gate_div, closed_min, use_loop_below_gate=True, G=None,
                 mutate=()):
    """The kernels' replay in float64: (w, m, v, closed) with closed[r, f] = element took the series.

    The series (J terms) is taken when s0 >= t_sat, k >= closed_min and every element with m != 0 that shares the
    element's LANE (f % G; G = None: every element decides alone) has sqrt(v) >= eps r^-kmax / gate_div; otherwise
    the exact per-step loop truncated at kmax steps.  `mutate` names deliberate errors (MUTATIONS);
    use_loop_below_gate = False is "no_gate"."""
    w, m, v = (np.atleast_2d(np.array(a, np.float64)) for a in (w, m, v))
    assert all(x in MUTATIONS for x in mutate)
    mutate = set(mutate) | (set() if use_loop_below_gate else {"no_gate"})
    b1, b2, lr, eps = f32(b1), f32(b2), f32(lr), f32(eps)
    kmax, t_sat = host_consts(b1, b2)
    r = math.sqrt(b2)
    kk = min(k, kmax)
    live = m != 0.0
    sv = np.sqrt(v)
    ok = ~live | (sv >= eps * r ** -kmax / gate_div) | ("no_gate" in mutate)
    if G is not None:  # a lane holding one element below the gate takes the loop for all of its elements
        for gl in range(min(G, w.shape[1])):
            ok[:, gl::G] = ok[:, gl::G].all(axis=1, keepdims=True)
    by_step = (s0 >= t_sat or "no_t_sat" in mutate) and (k >= closed_min or "no_closed_min" in mutate)
    closed = live & ok & by_step
    loop = live & ~closed
    # the series: lr (m / sqrt v) sum_j (-e)^j G_j(k), e = eps / sqrt v, G_j(k) = z_j (1 - z_j^k) / (1 - z_j)
    ks = k if "series_k_for_kk" in mutate else kmax if "series_kmax_for_k" in mutate else kk
    terms = J - 1 if "drop_last_term" in mutate else J
    svs = np.where(closed, sv, 1.0)
    acc = np.zeros_like(w)
    for j in range(terms):
        z = b1 / r ** (j + 1)
        acc += (-eps / svs) ** j * (z * (1.0 - z ** ks) / (1.0 - z))
    w_closed = w - lr * (m / svs) * acc
    w_loop, _, _ = dense_zero_steps(w, np.where(loop, m, 0.0), np.where(loop, v, 1.0), s0, kk, lr, b1, b2, eps)
    w = np.where(closed, w_closed, np.where(loop, w_loop, w))
    kd = kk if "state_kk_for_k" in mutate else k
    return w, m * b1 ** kd, v * b2 ** kd, closed


def seeded_rows(rows, d, b1, b2, eps, seed):
    """(w, m, v, class_id) of a [rows, d] table, all fp32 values; class_id[r] is one of ZERO_M ... PADDED.

      ZERO_M   m = 0, v > 0: must not move (row 0, the pad row, is one of them, with w = 0)
      TYPICAL  v ~ 1e-6 ... 1e-3 (log-uniform), |m| / sqrt(v) in [0.5, 5]
      GATE     every element at sqrt(v) = f * sv_min for f in GATE_FACTORS and both paths' sv_min, |m| / sqrt(v) in
               [2, 5]: with beta1 = 0.9 a long replay moves such a row by 0.18 ... 0.45 (float64), within [0.05, 0.5]
      MIXED    a typical row with ONE element at 0.05 sv_min of a path (under both gates): the kernels decide per lane,
               so the lane sharing that element takes the loop, the row's other lanes the series
      PADDED   (d % G != 0) the real elements of the lanes that also hold padding slots sit 1.1x above the batched
               gate: the padding (m = v = 0 in registers) must not count against the lane
    """
    rng = np.random.default_rng(seed)
    G, _ = lane_geometry(d)
    w = (rng.random((rows, d)) - 0.5).astype(np.float32) * np.float32(0.5)
    sv = np.exp(rng.uniform(math.log(1e-3), math.log(10 ** -1.5), (rows, d)))
    ratio = rng.uniform(0.5, 5.0, (rows, d)) * rng.choice([-1.0, 1.0], (rows, d))
    cls = np.full(rows, TYPICAL, np.int64)
    cls[:8] = ZERO_M
    w[0] = 0
    nxt = 8
    gates = {p: sv_min(p, b1, b2, eps) for p in PATHS}
    for p in PATHS:
        for fac in GATE_FACTORS:
            cls[nxt] = GATE
            sv[nxt] = fac * gates[p]
            ratio[nxt] = np.sign(ratio[nxt]) * rng.uniform(2.0, 5.0, d)
            nxt += 1
    for p in PATHS:
        for f in (3 % d, d - 1):
            cls[nxt] = MIXED
            sv[nxt, f] = 0.05 * gates[p]
            ratio[nxt, f] = math.copysign(4.0, ratio[nxt, f])
            nxt += 1
    if d % G:
        for _ in range(4):
            cls[nxt] = PADDED
            lanes = np.arange(d) % G >= d % G  # these lanes' last slot is padding
            sv[nxt, lanes] = 1.1 * gates["batched"]
            ratio[nxt, lanes] = np.sign(ratio[nxt, lanes]) * 4.0
            nxt += 1
    assert nxt + 16 <= rows, "too few rows for the classes and a body of typical rows"
    v = (sv * sv).astype(np.float32)
    m = (ratio * np.sqrt(v.astype(np.float64))).astype(np.float32)
    m[cls == ZERO_M] = 0
    return w, m, v, cls


def route_counts(path, m, v, cls, d, s0, k, b1, b2, eps):
    """How many seeded rows hold elements on each side of the route decision `path` makes for (s0, k): a dict
    closed / loop (rows with at least one element there), below_gate (rows with a live element under sv_min),
    still (rows with m = 0) — what a test asserts before it launches anything."""
    G, _ = lane_geometry(d)
    z = np.zeros(np.shape(m))
    closed = closed_model(z, m, v, s0, k, 0.0, b1, b2, eps, G=G, **path_kw(path, b1, b2))[3]
    live = np.asarray(m) != 0
    below = live & (np.sqrt(np.asarray(v, np.float64)) < sv_min(path, b1, b2, eps))
    return dict(closed=int(closed.any(axis=1).sum()), loop=int((live & ~closed).any(axis=1).sum()),
                below_gate=int(below.any(axis=1).sum()), still=int((~live).all(axis=1).sum()),
                by_class={CLASS_NAMES[c]: int((cls == c).sum()) for c in range(5)})
