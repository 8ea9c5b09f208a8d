"""Adagrad on the CPU: the premise of the fused kernels (a dense torch.optim.Adagrad leaves every row outside the batch
bit-unchanged, so there is nothing to replay), the numpy model the kernels are held to (tests/adagrad_model.py) against
torch's own CPU kernels, and what needs no device: the checks of bpr_set_optimizer, the struct mirror, and
bpr_opt_plan.h in a program of its own under the host sanitizers."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adagrad_model as am

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "revisit-bpr_amd" / "csrc"
U, I, D, B, STEPS = 40, 30, 20, 16, 6
REG = {"user": 0.0016, "item": 0.0001, "neg": 0.00375}
ALPHAS = (0.0016, 0.0001, 0.00375)
LR, EPS = 0.05, 1e-10
CASES = [(ld, iav) for ld in (0.0, 0.1) for iav in (0.0, 0.5)]


def batches(seed):
    """Triples with users and items repeated inside a batch, and the pad user / pad item present."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(STEPS):
        u = rng.integers(1, U, B)
        i = rng.integers(1, I, B)
        j = rng.integers(1, I, B)
        u[1] = u[0]
        i[3] = i[2]
        j[5] = i[4]
        u[7] = 0
        i[8] = 0
        out.append((u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)))
    return out


def torch_run(lr_decay, iav, item_bias):
    """The mirror's dense PyTorch restatement with a stock torch.optim.Adagrad on CPU tensors: per step the tables and
    `sum` before and after."""
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF, set_backend

    set_backend("torch")
    try:
        torch.manual_seed(3)
        model = BPR(fuse_forward=True, reg_alphas=REG,
                    logits_model=MF(torch.nn.Embedding(U, D, padding_idx=0), torch.nn.Embedding(I, D, padding_idx=0),
                                    item_bias=item_bias))
        if item_bias:
            with torch.no_grad():
                model.logits_model._item_bias.copy_(torch.linspace(-0.1, 0.1, I))
        opt = torch.optim.Adagrad(model.parameters(), lr=LR, lr_decay=lr_decay, eps=EPS, initial_accumulator_value=iav)
        lm = model.logits_model
        prm = {"P": lm._user_emb.weight, "Q": lm._item_emb.weight}
        if item_bias:
            prm["b"] = lm._item_bias

        def snap():
            return ({k: p.detach().numpy().copy() for k, p in prm.items()},
                    {k: opt.state[p]["sum"].numpy().copy() for k, p in prm.items()})

        model.train()
        trace = []
        for u, i, j in batches(seed=5):
            before = snap()
            out = model({"user": torch.from_numpy(u).long(), "item": torch.from_numpy(i).long()[:, None],
                         "neg": torch.from_numpy(j).long()[:, None]})
            out["loss"].backward()
            grads = {k: p.grad.detach().numpy().copy() for k, p in prm.items()}
            opt.step()
            opt.zero_grad()
            trace.append((u, i, j, before, snap(), grads))
        steps = {k: float(opt.state[p]["step"]) for k, p in prm.items()}
        return trace, steps
    finally:
        set_backend("hip")


_RUNS = {}


def run(lr_decay, iav, item_bias):
    key = (lr_decay, iav, item_bias)
    if key not in _RUNS:
        _RUNS[key] = torch_run(*key)
    return _RUNS[key]


# ---- 1. the structural claim --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr_decay,iav", CASES)
@pytest.mark.parametrize("item_bias", [False, True])
def test_dense_adagrad_leaves_rows_outside_the_batch_bit_unchanged(lr_decay, iav, item_bias):
    """Six steps of a DENSE torch.optim.Adagrad: after each, every row that is not in the batch — and the pad embedding
    rows, whose gradient torch drops — is bit-identical in weight and in `sum` to its value before the step.  This is
    the exactness the fused kernels' "no replay, no flush" rests on."""
    trace, steps = run(lr_decay, iav, item_bias)
    assert set(steps.values()) == {float(STEPS)}
    for u, i, j, (w0, s0), (w1, s1), _ in trace:
        ru, ri, rb = am.touched_rows(u, i, j)
        for k, rows, n in (("P", ru, U), ("Q", ri, I)) + ((("b", rb, I),) if item_bias else ()):
            rest = np.setdiff1d(np.arange(n), rows)
            assert rest.size > 0 and rows.size > 0
            assert np.array_equal(w0[k][rest].view(np.int32), w1[k][rest].view(np.int32)), k
            assert np.array_equal(s0[k][rest].view(np.int32), s1[k][rest].view(np.int32)), k
            assert not np.array_equal(w0[k][rows], w1[k][rows])  # (the batch's rows did move)


# ---- 2. the numpy model against torch on the touched rows -----------------------------------------------------------
SUM_ULP_SEEN, STEP_ULP_SEEN = 1, 2  # the largest distances measured on these inputs (see the docstring below)


@pytest.mark.parametrize("lr_decay,iav", CASES)
@pytest.mark.parametrize("item_bias", [False, True])
def test_numpy_lines_are_torchs_adagrad_step(lr_decay, iav, item_bias):
    """The model's three fp32 lines (adagrad_model.update) against torch's CPU kernels, fed the SAME gradient — torch's
    own p.grad — from torch's own pre-step state, for each of the six steps, on the touched rows of every table.

    Bit equality does not hold.  Measured with the installed torch (CPU, single-tensor path), per step, the worst of
    the eight cases:
      * `sum`: 1 ulp — torch's CPU addcmul contracts sum + g * g into one fused multiply-add, the model (and the
        kernels, built without contraction) round the product first; bit-equal while sum is still 0;
      * the weights: 2 units of adagrad_model.step_ulps, i.e. one rounding of the step counted in the finer spacing
        below a binade boundary — torch's CPU addcdiv rounds (clr * g) / std, while the order the kernels use (and
        torch's GPU addcdiv kernel) is clr * (g / std); from sum = 0 the CPU order reproduces torch's bits exactly.
    Asserted: twice the measured figures (2 ulp, 4 units)."""
    trace, _ = run(lr_decay, iav, item_bias)
    worst_w, worst_s = 0.0, 0
    for t, (u, i, j, (w0, s0), (w1, s1), g) in enumerate(trace, start=1):
        ru, ri, rb = am.touched_rows(u, i, j)
        for k, rows in (("P", ru), ("Q", ri)) + ((("b", rb),) if item_bias else ()):
            c = am.clr(LR, lr_decay, t)
            w, sm = w0[k].copy(), s0[k].copy()
            am.update(w, sm, g[k], rows, c, EPS)
            worst_w = max(worst_w, am.step_ulps(w, w1[k], w0[k]))
            worst_s = max(worst_s, am.ulp_distance(sm, s1[k]))
    print(f"adagrad lines vs torch: lr_decay={lr_decay} iav={iav} bias={item_bias}: sum {worst_s} ulp, w {worst_w}")
    assert worst_s <= 2 * SUM_ULP_SEEN and worst_w <= 2 * STEP_ULP_SEEN


@pytest.mark.parametrize("lr_decay,iav", CASES)
@pytest.mark.parametrize("item_bias", [False, True])
def test_numpy_model_step_follows_torch(lr_decay, iav, item_bias):
    """The whole model step — the oracle's batch gradient (accumulated in double, rounded once) into the three lines —
    against torch's step from the same state.  The gradients differ by fp32 summation order, so this is held to the
    one-step tolerance of tests/test_gpu_parity.py (its header: 2e-6 * max(1, |w|)), not to bits."""
    trace, _ = run(lr_decay, iav, item_bias)
    for t, (u, i, j, (w0, s0), (w1, s1), _) in enumerate(trace, start=1):
        P, Q = w0["P"].copy(), w0["Q"].copy()
        b = w0["b"].copy() if item_bias else None
        sums = {k: v.copy() for k, v in s0.items()}
        am.step(P, Q, b, sums, u, i, j, LR, lr_decay, EPS, t, ALPHAS)
        for k, got in (("P", P), ("Q", Q)) + ((("b", b),) if item_bias else ()):
            for a, w in ((got, w1[k]), (sums[k], s1[k])):
                err = np.abs(a.astype(np.float64) - w) / np.maximum(1.0, np.abs(w))
                assert err.max() <= 2e-6, (t, k, err.max())


def test_model_clr_is_torchs():
    """clr of step t from Python floats, rounded once; the ABI's (float lr, float lr_decay) is within one rounding."""
    for t in (1, 2, 5, 1000):
        want = np.float32(0.05 / (1 + (t - 1) * 0.1))
        assert am.clr(0.05, 0.1, t) == want
        assert abs(float(am.clr(0.05, 0.1, t, abi=True)) - float(want)) <= 2 * np.spacing(want)
    assert am.clr(0.05, 0.0, 7) == np.float32(0.05)


# ---- 3. refusals and plumbing that need no GPU ----------------------------------------------------------------------
def _params(**kw):
    from revisit_bpr import native

    vals = dict(lr=0.05, momentum=0.0, dampening=0.0, nesterov=0, beta1=0.9, beta2=0.999, eps=1e-10, alpha=0.99,
                lr_decay=0.0)
    vals.update(kw)
    return native.OptParams(**vals)


def test_set_optimizer_checks_need_no_device():
    """bpr_set_optimizer looks at the kind and its hyper-parameters before the ctx: the new kind is known (the call
    gets as far as the missing ctx), kind 5 is not, lr_decay < 0 and lr_decay with Adam are refused."""
    from revisit_bpr import native

    lib = native.load()
    assert native.OPT_ADAGRAD == 4

    def call(kind, **kw):
        rc = lib.bpr_set_optimizer(None, kind, ctypes.byref(_params(**kw)))
        return rc, lib.bpr_last_error().decode()

    rc, msg = call(native.OPT_ADAGRAD, lr_decay=0.1)
    assert rc == -1 and "ctx is NULL" in msg
    rc, msg = call(native.OPT_ADAGRAD + 1)
    assert rc == -1 and "unknown optimizer kind" in msg
    rc, msg = call(native.OPT_ADAGRAD, lr_decay=-0.1)
    assert rc == -1 and "lr_decay must be >= 0" in msg
    rc, msg = call(native.OPT_ADAGRAD, lr_decay=float("nan"))
    assert rc == -1 and "lr_decay" in msg
    for kind in (native.OPT_SGD, native.OPT_MOMENTUM, native.OPT_ADAM, native.OPT_RMSPROP):
        rc, msg = call(kind, lr_decay=0.1)
        assert rc == -1 and "lr_decay belongs to BPR_OPT_ADAGRAD" in msg
        rc, msg = call(kind)
        assert rc == -1 and "ctx is NULL" in msg
    assert lib.bpr_set_optimizer(None, native.OPT_ADAGRAD, None) == -1


def test_struct_mirror_matches_the_header():
    """native.OptParams against struct bpr_opt_params: the same fields in the same order, lr_decay last, 36 bytes."""
    from revisit_bpr import native

    text = (ROOT / "include" / "bprcore.h").read_text()
    body = re.search(r"typedef struct bpr_opt_params \{(.*?)\} bpr_opt_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    assert [(n, ctypes_of[c]) for n, c in fields] == list(native.OptParams._fields_)
    assert fields[-1] == ("lr_decay", "float")
    assert ctypes.sizeof(native.OptParams) == 4 * len(fields) == 36
    assert re.search(r"BPR_OPT_ADAGRAD\s*=\s*4\b", text)


def test_mirror_refuses_what_is_not_fused():
    """_configure_optimizer's refusals for the new kind, in the existing style (no engine is needed to get there)."""
    from revisit_bpr.models import BPR
    from revisit_bpr.models.bpr import MF
    from revisit_bpr.models.bpr import model as model_mod

    assert model_mod._OPT_KINDS["Adagrad"] == 4
    m = BPR(MF(torch.nn.Embedding(4, 8, padding_idx=0), torch.nn.Embedding(4, 8, padding_idx=0)))
    for kw in (dict(weight_decay=0.1), dict(maximize=True), dict(differentiable=True)):
        opt = torch.optim.Adagrad(m.parameters(), lr=0.05, **kw)
        with pytest.raises(NotImplementedError):
            m._configure_optimizer(opt, opt.param_groups[0])


def test_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """bpr_opt_plan.h is plain C++: built into a program of its own with -fsanitize=address,undefined,
    tests/adagrad_plan_check.cpp runs clean (the checks of bpr_set_optimizer, clr against a long-double restatement)."""
    exe = tmp_path / "adagrad_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(CSRC), str(ROOT / "tests" / "adagrad_plan_check.cpp"), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
