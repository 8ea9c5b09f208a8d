"""torch.optim.Adagrad on the BPR-MF tables, restated row-sparse in numpy fp32 — the model the Adagrad kernels are held to
(tests/test_gpu_adagrad.py) and that tests/test_adagrad_model_cpu.py holds to torch itself.

One step t (1-based) on a batch of (u, i, j) triples:
  * the batch gradient is the oracle's (`oracle.dense_grad`: every triple evaluated at the pre-step rows, duplicates
    summed, the pad embedding rows' gradients dropped), as `oracle.step` forms it for the other kinds;
  * clr = lr / (1 + (t - 1) * lr_decay), computed in double and rounded to float once — torch computes it on Python
    floats and hands it to its fp32 kernel as a scalar;
  * on the TOUCHED rows only, torch's single-tensor lines in fp32, each operation rounded on its own:
        sum = sum + g * g;   std = sqrt(sum) + eps;   w = w - clr * (g / std)
    A row outside the batch has g = 0: sum + 0 * 0 and w - clr * 0 / std leave it as it is, bit for bit, which is why the
    dense optimizer needs no replay (test 1 of the CPU file checks that on torch itself).

The C ABI carries lr and lr_decay as floats: `clr(..., abi=True)` is the library's scalar (the float values widened to
double), which may sit one rounding of lr (6e-8 relative) away from torch's.
"""
import numpy as np

import oracle

F = np.float32


def clr(lr, lr_decay, t, abi=False):
    """The decayed rate of 1-based step t, as a float32."""
    if abi:
        lr, lr_decay = float(F(lr)), float(F(lr_decay))
    return F(float(lr) / (1.0 + (t - 1) * float(lr_decay)))


def touched_rows(users, pos, neg, pad_user=0, pad_item=0):
    """(user rows, item rows, bias entries) a batch moves.  The pad embedding rows never move; the pad item's bias is
    an ordinary parameter."""
    u = np.unique(users)
    it = np.unique(np.concatenate([pos, neg]))
    return u[u != pad_user], it[it != pad_item], it


def update(w, s, g, rows, c, eps, cpu_order=False):
    """torch's three lines on w[rows], s[rows] in place (fp32, unfused).  The last line is w - clr * (g / std), the
    order of the library's kernels and of torch's GPU addcdiv kernel; torch's CPU addcdiv kernel rounds
    (clr * g) / std instead (`cpu_order`), one rounding of the step apart."""
    g = g[rows].astype(F)
    sr = s[rows] + g * g
    std = np.sqrt(sr) + F(eps)
    w[rows] = w[rows] - ((F(c) * g) / std if cpu_order else F(c) * (g / std))
    s[rows] = sr


def step(P, Q, b, sums, users, pos, neg, lr, lr_decay, eps, t, alphas=(0.0, 0.0, 0.0), pad_user=0, pad_item=0,
         abi=False):
    """One Adagrad step in place.  P [U, d], Q [I, d], b [I] or None; sums = dict(P=, Q=, b=) of the same shapes."""
    gP, gQ, gb = oracle.dense_grad(P, Q, b, users, pos, neg, alphas, pad_user, pad_item)
    ru, ri, rb = touched_rows(users, pos, neg, pad_user, pad_item)
    c = clr(lr, lr_decay, t, abi)
    update(P, sums["P"], gP, ru, c, eps)
    update(Q, sums["Q"], gQ, ri, c, eps)
    if b is not None:
        update(b, sums["b"], gb, rb, c, eps)
    return ru, ri, rb


def new_sums(P, Q, b, initial_accumulator_value=0.0):
    s = {"P": np.full_like(P, initial_accumulator_value), "Q": np.full_like(Q, initial_accumulator_value)}
    if b is not None:
        s["b"] = np.full_like(b, initial_accumulator_value)
    return s


def step_ulps(got, want, before):
    """Largest |got - want| in units in the last place of the step's operands: the update w - clr * (g / std) subtracts
    two rounded quantities, and where it cancels (|w| far below the step) an ulp of the RESULT says nothing — one
    rounding of the step is thousands of them.  The unit is spacing(max(|w before|, |w after|, |step|))."""
    got, want, before = (np.asarray(x, F) for x in (got, want, before))
    scale = np.maximum(np.maximum(np.abs(before), np.abs(want)), np.abs(want - before))
    unit = np.spacing(np.maximum(scale, np.finfo(F).tiny).astype(F)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want) / unit).max()) if got.size else 0.0


def ulp_distance(a, b):
    """Largest distance in units in the last place between two float32 arrays (same sign assumed where it matters:
    the integer images of IEEE floats are ordered)."""
    a = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, F).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return int(np.abs(a - b).max()) if a.size else 0
