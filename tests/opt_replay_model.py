"""The lazy replay of the non-Adam stateful optimizers in float64, at every register layout of the STRICT kernels.

`bpr_bind_tables` (bprcore.hip, "c->G = d <= 128 ? 32 : 64" and the two lines after it) picks one of six layouts from the
embedding dim: G lanes per row, E elements per lane, element e of lane gl being feature e * G + gl and features >= d
padding.  Every STRICT kernel exists once per layout, and under a stateful optimizer each of them replays the
zero-gradient steps a dense torch.optim applied to rows nobody touched (`opt_replay_row`, `opt_replay`, `catch_up_row`
in bpr_opt.h).  This module states, without torch and without a GPU:

  * `layout(d)` and DIMS, the dims that put every layout at its smallest and its largest d and at a partial last element;
  * KINDS, the momentum / Nesterov / dampening / RMSprop / RMSprop-with-momentum configurations;
  * `seeded_state`, the tables the GPU tests write into the engine;
  * `replay_float64`, the k zero-gradient steps as a step-by-step loop (the kernels use geometric sums);
  * MUTANTS, that loop with one deliberate defect each, so that tests/test_opt_replay_cpu.py can show on the CPU that
    the seeded tables tell a right replay from each of them with a tenfold margin.

Adam has a model of its own, tests/adam_replay_model.py.
"""
import math

import numpy as np

DIMS = [1, 32, 33, 64, 65, 100, 129, 256, 257, 300, 512, 513, 1000, 1024]
GAPS = (1, 7, 60)
ROWS = 96
STILL = tuple(range(8))  # rows seeded with m = 0; row 0 is the pad row, all zero

# lrs as test_gpu_parity.test_stateful_optimizers_long_horizon_vs_dense_oracle
KINDS = {
    "momentum": dict(kind=1, lr=0.01, momentum=0.9),
    "nesterov": dict(kind=1, lr=0.01, momentum=0.9, nesterov=True),
    "momentum_damp": dict(kind=1, lr=0.02, momentum=0.5, dampening=0.3),
    "rmsprop": dict(kind=3, lr=0.0005, alpha=0.9),
    "rmsprop_mom": dict(kind=3, lr=0.0003, alpha=0.9, momentum=0.8),
}


def f32(x):
    return float(np.float32(x))


def layout(d):
    """(G, E) of bpr_bind_tables:

        d          G   E
        1-32       32  1
        33-64      32  2
        65-128     32  4
        129-256    64  4
        257-512    64  8
        513-1024   64  16
    """
    assert 1 <= d <= 1024
    G = 32 if d <= 128 else 64
    per_lane = -(-d // G)
    E = (1 if per_lane <= 1 else 2 if per_lane <= 2 else 4) if G == 32 else (4 if per_lane <= 4 else 8 if per_lane <= 8 else 16)
    return G, E


def has_m(kind):
    c = KINDS[kind]
    return c["kind"] == 1 or c.get("momentum", 0.0) > 0


def has_v(kind):
    return KINDS[kind]["kind"] == 3


def seeded_state(kind, rows, d, seed):
    """dict w, m, v ([rows, d]), b, mb, vb ([rows]), all fp32, and still / still_b (bool [rows]: m = 0 / mb = 0); m / mb are None for a kind
    without a buffer, v / vb for a kind without a second moment.

      w   rand_problem's scale times four, as the long-horizon test trains on: uniform in +-8 / d
      m   a gradient: |m| log-uniform in [0.05, 0.5], random sign.  Under RMSprop with momentum the buffer sums
          g / sqrt(v) with weight 1 / (1 - mu), so there |m| is log-uniform in [1, 8]
      v   a squared gradient: sqrt(v) log-uniform in [0.05, 0.5]
      rows STILL carry m = 0 (and v > 0): they must not move at all; row 0, the pad row, is zero throughout
      b   the item bias seeded like one column, except that b[0] is a live entry: the bias has no padding index
    """
    rng = np.random.default_rng(seed)
    lo, hi = (1.0, 8.0) if kind == "rmsprop_mom" else (0.05, 0.5)

    def draw(shape):
        w = ((rng.random(shape) - 0.5) / d * 16).astype(np.float32)
        m = (np.exp(rng.uniform(math.log(lo), math.log(hi), shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
        v = (np.exp(rng.uniform(math.log(0.05), math.log(0.5), shape)) ** 2).astype(np.float32)
        return w, m, v

    w, m, v = draw((rows, d))
    b, mb, vb = draw((rows,))
    still = np.zeros(rows, bool)
    still[list(STILL)] = True
    m[still] = 0
    mb[still] = 0
    mb[0] = np.float32(math.copysign(lo * 2, 1.0))  # b[0] is live
    w[0] = 0
    v[0] = 0
    out = dict(w=w, m=m if has_m(kind) else None, v=v if has_v(kind) else None,
               b=b, mb=mb if has_m(kind) else None, vb=vb if has_v(kind) else None, still=still)
    out["still_b"] = still.copy()
    out["still_b"][0] = False
    return out


def replay_float64(kind, w, m, v, k, cfg=None, drop_nesterov_mu=False, keep_v=False, hold_row=False):
    """k zero-gradient steps of torch.optim.SGD(momentum) / RMSprop, one after the other, in float64.  Returns (w, m, v)
    (m, v None where given None).  The keyword switches are the defects of MUTANTS.

    SGD, g = 0, not the first step:  buf <- mu buf + (1 - dampening) 0;  w <- w - lr (nesterov ? 0 + mu buf : buf)
    RMSprop, g = 0:  v <- alpha v;  momentum > 0:  buf <- mu buf + 0 / avg;  w <- w - lr buf;  else  w <- w - lr 0 / avg
    """
    cfg = KINDS[kind] if cfg is None else cfg
    w = np.array(w, np.float64)
    m = None if m is None else np.array(m, np.float64)
    v = None if v is None else np.array(v, np.float64)
    lr, mu = f32(cfg["lr"]), f32(cfg.get("momentum", 0.0))
    for _ in range(k):
        if cfg["kind"] == 1:
            m *= mu
            w -= lr * (m if (not cfg.get("nesterov") or drop_nesterov_mu) else mu * m)
        else:
            if not keep_v:
                v *= f32(cfg["alpha"])
            if mu > 0:
                m *= mu
                if not hold_row:
                    w -= lr * m
    return w, m, v


def replay_tables(kind, s, k, cfg=None, **defect):
    """`replay_float64` on a seeded table and its bias: dict w, m, v, b, mb, vb (float64)."""
    w, m, v = replay_float64(kind, s["w"], s["m"], s["v"], k, cfg, **defect)
    b, mb, vb = replay_float64(kind, s["b"], s["mb"], s["vb"], k, cfg, **defect)
    return dict(w=w, m=m, v=v, b=b, mb=mb, vb=vb)


def _skip_feature(f):
    def run(kind, s, k, cfg=None):
        out = replay_tables(kind, s, k, cfg)
        for n in ("w", "m", "v"):
            if out[n] is not None:
                out[n][:, f(s["w"].shape[1])] = s[n][:, f(s["w"].shape[1])]
        return out
    return run


def _skip_bias(kind, s, k, cfg=None):
    out = replay_tables(kind, s, k, cfg)
    for n in ("b", "mb", "vb"):
        if out[n] is not None:
            out[n] = np.array(s[n], np.float64)
    return out


# name -> (which kinds, which dims, the defective replay of a whole table)
MUTANTS = {
    "gap_minus_one": (list(KINDS), lambda d: True, lambda kind, s, k, cfg=None: replay_tables(kind, s, k - 1, cfg)),
    "gap_plus_one": (list(KINDS), lambda d: True, lambda kind, s, k, cfg=None: replay_tables(kind, s, k + 1, cfg)),
    "last_feature_skipped": (list(KINDS), lambda d: True, _skip_feature(lambda d: d - 1)),
    "feature_G_skipped": (list(KINDS), lambda d: d > layout(d)[0], _skip_feature(lambda d: layout(d)[0])),
    "nesterov_mu_dropped": (["nesterov"], lambda d: True,
                            lambda kind, s, k, cfg=None: replay_tables(kind, s, k, cfg, drop_nesterov_mu=True)),
    "rmsprop_v_not_decayed": (["rmsprop", "rmsprop_mom"], lambda d: True,
                              lambda kind, s, k, cfg=None: replay_tables(kind, s, k, cfg, keep_v=True)),
    "rmsprop_mom_row_held": (["rmsprop_mom"], lambda d: True,
                             lambda kind, s, k, cfg=None: replay_tables(kind, s, k, cfg, hold_row=True)),
    "bias_skipped": (list(KINDS), lambda d: True, _skip_bias),
}
