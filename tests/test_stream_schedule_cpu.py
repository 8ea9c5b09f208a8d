"""`fast.resolve_schedule` — everything `fast.StreamTrainer` decides about its launches and its snapshot, as a pure
function — swept on the CPU over shapes, learning rates, ranks and samplers.

The constructor used to decide `launch_split` on the whole refresh period and then `refresh_lag` / `hot_lds` on the
HALVED launch: for LAG_BUDGET / 2 < lr x period <= LAG_BUDGET the defaults contradicted each other ("launch_split > 1
needs refresh_lag 0") and the LDS tier came on at a rate its own docstring calls outside.  `_parent` below restates
those rules; the sweep holds the resolver to them wherever they were consistent and to the reference's schedule
wherever they were not.
"""
import itertools
import math
import warnings

import pytest

from revisit_bpr import fast

ITEMS = (2, 300, 1501, 5000, 20109, 41141, 65536, 92090, 131071)
DIMS = (1, 8, 32, 64, 128, 256, 512, 1024)
BATCHES = (1, 128, 512, 2048)
WORLDS = (1, 2, 8)
SAMPLERS = ("adaptive", "uniform")
GEOMETRIC = tuple(1e-4 * 10.0 ** (4.0 * k / 199) for k in range(200))  # 1e-4 .. 1


def _period(I, B):
    return max(1, int(I * math.log(I) / B)) * B


def _edges(period):
    """The two ends of the window LAG_BUDGET / 2 < lr x period <= LAG_BUDGET, each one ulp below and above."""
    out = []
    for e in (fast.LAG_BUDGET / (2 * period), fast.LAG_BUDGET / period):
        out += [math.nextafter(e, 0.0), math.nextafter(e, math.inf)]
    return tuple(out)


def _sizes(period):
    """A triple list longer than a refresh period, and one shorter than HALF of it (the chunk is then the list)."""
    return 3 * period + 1, max(1, period // 3)


def _parent(I, d, n, B, lr, sampler, world, item_sync, cadence="job", refresh_split=1, launch_split="auto",
            refresh_lag="auto", refresh_cus=0, hot_lds="auto"):
    """The constructor's rules before `resolve_schedule` (valid argument types assumed): the tuple (launch_split,
    chunk, refresh_lag, refresh_cus, hot_lds) or "raises".  refresh_cus counts only beside a lagged snapshot."""
    world, period, auto_lag = max(world, 1), _period(I, B), refresh_lag == "auto"
    per = world if cadence == "job" else 1 if cadence == "rank" else fast.launches_per_period(lr, world, period)
    if launch_split == "auto":
        launch_split = 1 if (world > 1 or refresh_split != 1 or (not auto_lag and refresh_lag != 0.0)
                             or fast.lag_within_budget(lr, period)) else 2
    if launch_split > 1 and (item_sync or refresh_split != 1):
        return "raises"
    chunk = max(1, min(period // (per * refresh_split * launch_split), n))
    lds = fast.hot_lds_rows(lr, chunk, world) if hot_lds == "auto" else hot_lds
    if auto_lag:
        refresh_lag, refresh_cus = (fast.auto_schedule(I, d, chunk, lr=lr)
                                    if not item_sync and sampler == "adaptive" else (0.0, 0))
    lag = float(refresh_lag) if sampler == "adaptive" else 0.0
    if lag != 0.0 and launch_split > 1:
        return "raises"
    return launch_split, chunk, lag, refresh_cus if lag > 0.0 else 0, lds


def _tuple(s):
    return s.launch_split, s.chunk, s.refresh_lag, s.refresh_cus, s.hot_lds


@pytest.fixture(scope="module")
def sweep():
    """ONE pass over the grid with everything on "auto", no item reconciliation, cadence "job" (the constructor's
    default): per property the points that break it (at most a few are kept), and the parent's raising set."""
    bad = {k: [] for k in ("refuses", "values", "split", "budget", "uniform", "ranks", "chunk", "moved", "raised_to")}
    raised, tier_off, points = set(), 0, 0

    def note(key, *what):
        if len(bad[key]) < 5:
            bad[key].append(what)

    for I, B in itertools.product(ITEMS, BATCHES):
        period = _period(I, B)
        lrs = GEOMETRIC + _edges(period)
        for d, lr, world, sampler, n in itertools.product(DIMS, lrs, WORLDS, SAMPLERS, _sizes(period)):
            at = (I, d, B, lr, world, sampler, n)
            points += 1
            try:
                s = fast.resolve_schedule(I, d, n, B, lr, sampler=sampler, world=world)
            except ValueError as e:
                note("refuses", at, str(e))
                continue
            got = _tuple(s)
            if not (s.period == period and s.chunk >= 1 and s.launch_split in (1, 2) and s.refresh_lag in (0.0, 1.0)
                    and s.hot_lds in (0, fast.HOT_LDS_ROWS) and s.refresh_cus >= 0 and not s.warn_lag
                    and math.isfinite(s.refresh_lag)):  # (the only float of the answer)
                note("values", at, got)
            if s.launch_split > 1 and not (got[2:] == (0.0, 0, 0) and world == 1):
                note("split", at, got)
            if world == 1 and (s.refresh_lag >= 1.0 or s.hot_lds > 0) and not (
                    s.launch_split == 1 and fast.lag_within_budget(lr, s.chunk)):
                note("budget", at, got)
            if sampler == "uniform" and s.refresh_lag != 0.0:
                note("uniform", at, got)
            if world > 1 and s.launch_split != 1:
                note("ranks", at, got)
            if s.chunk != max(1, min(period // (s.per_period * 1 * s.launch_split), n)) or (
                    n >= period and s.chunk * s.launch_split > period) or s.per_period != world:
                note("chunk", at, got)
            want = _parent(I, d, n, B, lr, sampler, world, False)
            if want == "raises":
                raised.add(at)
                if got != (2, min(period // 2, n), 0.0, 0, 0):
                    note("raised_to", at, got)
            elif period < 2 and want[0] > 1:  # a period of ONE triple was "halved" into two launches of one triple
                if got != (1,) + want[1:]:
                    note("moved", at, got, want)
            elif want[0] > 1 and want[4] > 0:  # two launches of one snapshot with the tier on: the tier goes, only it
                tier_off += 1
                if got != want[:4] + (0,):
                    note("moved", at, got, want)
            elif got != want:
                note("moved", at, got, want)
    return {"bad": bad, "raised": raised, "tier_off": tier_off, "points": points}


def test_all_auto_never_refuses_and_answers_in_range(sweep):
    """Every default construction resolves: chunk >= 1, launch_split 1 or 2, refresh_lag 0 or 1, the tier off or
    HOT_LDS_ROWS, finite, no warning — at every grid point, the window's four edges included."""
    assert sweep["points"] == len(ITEMS) * len(BATCHES) * len(DIMS) * 204 * len(WORLDS) * 2 * 2
    assert not sweep["bad"]["refuses"], sweep["bad"]["refuses"]
    assert not sweep["bad"]["values"], sweep["bad"]["values"]


def test_split_means_the_reference_schedule(sweep):
    """launch_split > 1 => refresh_lag 0, no masked sort, tier off, one rank (no item_sync on this grid)."""
    assert not sweep["bad"]["split"], sweep["bad"]["split"]


def test_one_rank_one_budget(sweep):
    """A lagged snapshot or the LDS tier => one launch per period, and that launch inside LAG_BUDGET."""
    assert not sweep["bad"]["budget"], sweep["bad"]["budget"]


def test_uniform_sampler_never_lags_and_ranks_never_split(sweep):
    assert not sweep["bad"]["uniform"], sweep["bad"]["uniform"]
    assert not sweep["bad"]["ranks"], sweep["bad"]["ranks"]


def test_chunk_arithmetic(sweep):
    """chunk == max(1, min(period // (per_period x refresh_split x launch_split), n)); launch_split launches never
    exceed a period; cadence "job": one share per rank."""
    assert not sweep["bad"]["chunk"], sweep["bad"]["chunk"]


def test_nothing_else_moved(sweep):
    """Against `_parent`: where it raised, the answer is two launches of the reference's schedule — (2, min(period
    // 2, n), 0.0, 0, 0), i.e. (2, period // 2, 0.0, 0, 0) unless the triple list is shorter; where it answered two
    launches WITH the LDS tier (uniform sampler, or a shape that gains nothing from lag 1: the tier was judged on the
    halved launch) only the tier goes — "split means the reference's schedule" forbids it; a period of one triple
    (I = 2, batch 1) is no longer "halved"; everywhere else the tuple is the parent's, exactly.  The raising set is
    not empty and holds the two documented rates."""
    assert not sweep["bad"]["raised_to"], sweep["bad"]["raised_to"]
    assert not sweep["bad"]["moved"], sweep["bad"]["moved"]
    raised = sweep["raised"]
    print(f"parent raised at {len(raised)} of {sweep['points']} grid points; tier taken off two-launch periods at "
          f"{sweep['tier_off']} more")
    assert len(raised) > 0 and sweep["tier_off"] > 0
    assert all(at[4] == 1 and at[5] == "adaptive" for at in raised)  # one rank, a snapshot to lag
    # ... with a triple list of at least a period, only inside the window
    assert all(not fast.lag_within_budget(at[3], _period(at[0], at[2]))
               and fast.lag_within_budget(at[3], _period(at[0], at[2]) // 2)
               for at in raised if at[6] >= _period(at[0], at[2]))
    for I, d, B, lr in ((20109, 128, 512, 0.01), (92090, 256, 512, 0.001)):
        period = _period(I, B)
        n = 3 * period + 1
        assert _parent(I, d, n, B, lr, "adaptive", 1, False) == "raises"
        assert _tuple(fast.resolve_schedule(I, d, n, B, lr)) == (2, period // 2, 0.0, 0, 0)
    # the grid's own neighbours of lr 0.01 at the ML-20M shape (lr is geometric there, not 0.01 itself)
    assert any(at[:3] == (20109, 128, 512) and 0.0051 < at[3] <= 0.01 for at in raised)
    assert any(at[:3] == (92090, 256, 512) and at[3] < 0.0019 for at in raised)


def test_item_sync_and_cadences():
    """With an item reconciliation (any number of ranks, every cadence): never refuses, never splits, never lags;
    the tier by the cadence's own rule.  The parent refused one rank with an item_sync outside the budget
    ("launch_split > 1: one GPU"): that default now resolves to one launch."""
    lrs = GEOMETRIC[::8]
    refused = 0
    for (I, B), d, cadence in itertools.product(itertools.product(ITEMS, BATCHES), (8, 128, 1024), ("job", "rank", "auto")):
        period = _period(I, B)
        for lr, world, sampler, n in itertools.product(lrs + _edges(period), WORLDS, SAMPLERS, _sizes(period)):
            s = fast.resolve_schedule(I, d, n, B, lr, sampler=sampler, world=world, item_sync=True, cadence=cadence)
            per = world if cadence == "job" else 1 if cadence == "rank" else fast.launches_per_period(lr, world, period)
            chunk = max(1, min(period // per, n))
            assert _tuple(s) == (1, chunk, 0.0, 0, fast.hot_lds_rows(lr, chunk, world)), (I, d, B, lr, world, cadence, n)
            assert s.per_period == per and 1 <= per <= fast.MAX_CHUNKS_PER_RANK_SHARE * world
            want = _parent(I, d, n, B, lr, sampler, world, True, cadence=cadence)
            refused += want == "raises"
            assert want == "raises" and world == 1 or want == _tuple(s)
            # without an item_sync a world > 1 (a shard of a simulated job) keeps the parent's answer too
            t = fast.resolve_schedule(I, d, n, B, lr, sampler=sampler, world=world, cadence=cadence)
            want = _parent(I, d, n, B, lr, sampler, world, False, cadence=cadence)
            assert world == 1 or _tuple(t) == want
    assert refused > 0


# (I, d, launch, lr): (lag_within_budget, auto_schedule(lr=lr), hot_lds_rows at world 1 / 2 / 8, launches_per_period
# with the launch as the period at world 1 / 2 / 8) — computed from the commit before `resolve_schedule` existed:
# the ML-20M, MSD and Yelp item counts at batch 512, the full and the halved period
FROZEN = {
    (20109, 128, 199168, 0.001): (True, (1.0, 32), (512, 512, 512), (1, 1, 1)),
    (20109, 128, 99584, 0.001): (True, (1.0, 64), (512, 512, 512), (1, 1, 1)),
    (20109, 128, 199168, 0.005): (True, (1.0, 32), (512, 512, 0), (1, 1, 2)),
    (20109, 128, 99584, 0.005): (True, (1.0, 64), (512, 512, 0), (1, 1, 1)),
    (20109, 128, 199168, 0.01): (False, (0.0, 0), (0, 0, 0), (1, 1, 4)),
    (20109, 128, 99584, 0.01): (True, (1.0, 64), (512, 512, 0), (1, 1, 2)),
    (20109, 128, 199168, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 5, 20)),
    (20109, 128, 99584, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 3, 10)),
    (41141, 64, 436736, 0.001): (True, (1.0, 64), (512, 512, 512), (1, 1, 1)),
    (41141, 64, 218368, 0.001): (True, (1.0, 96), (512, 512, 512), (1, 1, 1)),
    (41141, 64, 436736, 0.005): (False, (0.0, 0), (0, 0, 0), (1, 2, 5)),
    (41141, 64, 218368, 0.005): (False, (0.0, 0), (0, 512, 0), (1, 1, 3)),
    (41141, 64, 436736, 0.01): (False, (0.0, 0), (0, 0, 0), (1, 3, 9)),
    (41141, 64, 218368, 0.01): (False, (0.0, 0), (0, 0, 0), (1, 2, 5)),
    (41141, 64, 436736, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 8, 32)),
    (41141, 64, 218368, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 6, 22)),
    (92090, 256, 1052160, 0.001): (False, (0.0, 0), (0, 512, 0), (1, 1, 3)),
    (92090, 256, 526080, 0.001): (True, (1.0, 128), (512, 512, 0), (1, 1, 2)),
    (92090, 256, 1052160, 0.005): (False, (0.0, 0), (0, 0, 0), (1, 3, 11)),
    (92090, 256, 526080, 0.005): (False, (0.0, 0), (0, 0, 0), (1, 2, 6)),
    (92090, 256, 1052160, 0.01): (False, (0.0, 0), (0, 0, 0), (1, 6, 22)),
    (92090, 256, 526080, 0.01): (False, (0.0, 0), (0, 0, 0), (1, 3, 11)),
    (92090, 256, 1052160, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 8, 32)),
    (92090, 256, 526080, 0.05): (False, (0.0, 0), (0, 0, 0), (1, 8, 32)),
}


def test_helpers_frozen():
    """bench.py calls these directly and keeps its own copy of the split rule: their values may not move."""
    assert (fast.LAG_BUDGET, fast.STALENESS_BUDGET, fast.HOT_LDS_ROWS, fast.MAX_CHUNKS_PER_RANK_SHARE) == (2000.0, 4000.0, 512, 4)
    assert len(FROZEN) == 3 * 4 * 2
    for I, d, B in ((20109, 128, 512), (41141, 64, 512), (92090, 256, 512)):
        assert all((I, d, launch, lr) in FROZEN for launch in (_period(I, B), _period(I, B) // 2)
                   for lr in (0.001, 0.005, 0.01, 0.05))
    for (I, d, launch, lr), (inside, sched, lds, per) in FROZEN.items():
        assert fast.lag_within_budget(lr, launch) is inside
        assert fast.auto_schedule(I, d, launch, lr=lr) == sched
        assert tuple(fast.hot_lds_rows(lr, launch, w) for w in (1, 2, 8)) == lds
        assert tuple(fast.launches_per_period(lr, w, launch) for w in (1, 2, 8)) == per
        assert all(fast.launches_per_period(lr, w, launch, fast.STALENESS_BUDGET) == k for w, k in zip((1, 2, 8), per))
    assert fast.auto_schedule(20109, 128, 199168, lr=0.001) == (1.0, 32)
    assert fast.auto_schedule(92090, 256, 526080, lr=0.001) == (1.0, 128)


ML20M = dict(I=20109, d=128, n=9_700_000, batch_size=512)  # period 199,168: inside the budget up to lr 0.00502


def _raises(message, **kw):
    with pytest.raises(ValueError) as e:
        fast.resolve_schedule(**{**ML20M, "lr": 0.001, **kw})
    assert str(e.value) == message


def test_explicit_arguments_are_refused_as_before():
    """Every ValueError of the constructor's schedule arguments, with its message, for the inputs that met it."""
    _raises("refresh_lag must be in [0, 1] or 'auto'", refresh_lag="fast")
    for kw in (dict(refresh_lag=-0.1), dict(refresh_lag=1.5), dict(refresh_lag=0.0, refresh_split=0),
               dict(refresh_split=0)):
        _raises("refresh_lag must be in [0, 1], refresh_split >= 1", **kw)
    _raises("cadence must be 'job', 'rank' or 'auto'", cadence="epoch")
    _raises("launch_split must be an int >= 1 or 'auto'", launch_split="two")
    for kw in (dict(launch_split=2, item_sync=True), dict(launch_split=2, item_sync=True, world=2),
               dict(launch_split=2, refresh_split=2), dict(launch_split=3, refresh_split=2, refresh_lag=0.0)):
        _raises("launch_split > 1: one GPU, refresh_split 1", **kw)
    for lr, lag, split in itertools.product((0.001, 0.01, 0.05), (0.25, 1.0), (2, 4)):
        _raises("launch_split > 1 needs refresh_lag 0", lr=lr, launch_split=split, refresh_lag=lag)
    with pytest.raises(KeyError):
        fast.resolve_schedule(**ML20M, lr=0.001, sampler="popularity")
    # ... and no refusal the constructor did not have: the uniform sampler has no snapshot to lag
    s = fast.resolve_schedule(**ML20M, lr=0.001, sampler="uniform", launch_split=2, refresh_lag=1.0)
    assert _tuple(s)[:3] == (2, 199168 // 2, 0.0)


def test_explicit_lag_outside_the_budget_warns_as_before():
    """refresh_lag 1 given explicitly, adaptive sampler, no item_sync, lr x 2 x launch > LAG_BUDGET: honoured, with the
    warning flag; no flag inside the budget, for a fractional lag, the uniform sampler or an item_sync."""
    def flag(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the resolver itself never warns: the constructor does, on the flag
            return fast.resolve_schedule(**{**ML20M, "refresh_lag": 1.0, "refresh_cus": 64, **kw})

    for lr in (0.0051, 0.01, 0.05):
        s = flag(lr=lr)
        assert s.warn_lag and _tuple(s) == (1, 199168, 1.0, 64, 0)
        assert not flag(lr=lr, sampler="uniform").warn_lag and not flag(lr=lr, item_sync=True).warn_lag
        assert not flag(lr=lr, refresh_lag=0.5).warn_lag and flag(lr=lr, refresh_lag=0.5).refresh_lag == 0.5
    for lr in (0.001, 0.005):
        s = flag(lr=lr)
        assert not s.warn_lag and _tuple(s) == (1, 199168, 1.0, 64, fast.HOT_LDS_ROWS)
    assert flag(lr=0.0126, refresh_split=2).chunk == 99584 and flag(lr=0.0126, refresh_split=2).warn_lag  # the LAUNCH counts
    assert not flag(lr=0.01, refresh_split=2).warn_lag  # 0.01 x 2 x 99,584 = 1,992


def test_explicit_arguments_are_honoured():
    """Explicit values come back as given — against `_parent` over launch_split x refresh_lag x refresh_split x
    refresh_cus x hot_lds at three shapes and four rates, "raises" for "raises".  Two rules are new and asserted on
    their own: an explicit launch_split k > 1 makes refresh_lag "auto" 0 (the parent could refuse its own choice), and
    hot_lds "auto" then asks with the k launches that share the snapshot, not with one of them."""
    shapes = ((1501, 32, 256), (20109, 128, 512), (92090, 256, 512))
    for (I, d, B), lr, sampler, split, lag, rsplit, cus, lds in itertools.product(
            shapes, (0.001, 0.01, 0.05, 0.14), SAMPLERS, (1, 2, 3, "auto"), (0.0, 0.5, 1.0), (1, 2), (0, 64, -1),
            (0, 100, "auto")):
        period = _period(I, B)
        for n in _sizes(period):
            want = _parent(I, d, n, B, lr, sampler, 1, False, refresh_split=rsplit, launch_split=split,
                           refresh_lag=lag, refresh_cus=cus, hot_lds=lds)
            try:
                got = _tuple(fast.resolve_schedule(I, d, n, B, lr, sampler=sampler, refresh_split=rsplit,
                                                   launch_split=split, refresh_lag=lag, refresh_cus=cus, hot_lds=lds))
            except ValueError:
                got = "raises"
            if want != "raises" and want[0] > 1 and lds == "auto":  # the tier: by the period, not by the launch
                span = min(period, want[1] * want[0])
                want = want[:4] + (0 if split == "auto" else fast.hot_lds_rows(lr, span),)
            assert got == want, (I, d, B, lr, sampler, split, lag, rsplit, cus, lds, n, got, want)
    # explicit launch_split, refresh_lag "auto": lag 0 at every rate, inside the budget included
    for lr in (0.001, 0.005, 0.0075, 0.01, 0.05):
        s = fast.resolve_schedule(**ML20M, lr=lr, launch_split=2)
        assert _tuple(s) == (2, 99584, 0.0, 0, fast.hot_lds_rows(lr, 199168))
        assert fast.resolve_schedule(**ML20M, lr=lr, launch_split=2, hot_lds=96).hot_lds == 96
    assert fast.resolve_schedule(**ML20M, lr=0.005, launch_split=2).hot_lds == fast.HOT_LDS_ROWS
    assert fast.resolve_schedule(**ML20M, lr=0.0075, launch_split=2).hot_lds == 0  # 2,988 for the period, 1,494 for the launch
    # all auto, an explicit tier: honoured beside the two launches
    assert _tuple(fast.resolve_schedule(**ML20M, lr=0.01, hot_lds=64)) == (2, 99584, 0.0, 0, 64)
    # refresh_cus "auto" beside an explicit lag: -1, resolved by `auto_refresh_cus` once the device is known
    assert fast.resolve_schedule(**ML20M, lr=0.001, refresh_lag=1.0, refresh_cus="auto").refresh_cus == -1
    assert fast.resolve_schedule(**ML20M, lr=0.001, refresh_lag=0.0, refresh_cus="auto").refresh_cus == 0
