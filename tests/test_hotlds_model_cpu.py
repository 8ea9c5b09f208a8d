"""The algorithm of the LDS tier of k_stream's hot block (tests/hotlds_model.py: a numpy restatement of the run
partition, the deal of runs to persistent workgroups and the private-delta algebra) on the CPU:

  * the zones partition [0, n) exactly — every triple in exactly one run, runs in order, zone boundaries on whole
    wave-loads, run lengths L / L/2 / L/4 — for every run length the API accepts and any tail share;
  * the deal hands every run to exactly one workgroup, wave-load by wave-load, a workgroup's own runs in rising order
    (so its short runs come last), consecutive wave-loads on different workgroups;
  * one workgroup == sequential SGD; with many workgroups nothing is lost whatever the interleaving (the table after
    the launch is the start plus the sum of every triple's update), a workgroup always sees its OWN updates of a hot
    row, and what it misses of the others' is bounded by their updates of that launch.
The HIP kernel is held to the oracle in tests/test_gpu_hotlds.py."""
import numpy as np
import pytest

import oracle
from hotlds_model import deal, run_launch, runs_of, two_half_stream, zones


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8, 12, 30])
@pytest.mark.parametrize("gpw", [1, 2])
def test_zones_partition_the_launch(L, gpw):
    rng = np.random.default_rng(L * 10 + gpw)
    for n in [1, 7, 16, 199_168, 40_928] + [int(x) for x in rng.integers(1, 60_000, 6)]:
        for tail in (0, 12, 25, 50):
            t1, t2 = zones(n, L, gpw, tail)
            assert 0 <= t1 <= t2 <= n and t1 % (L * gpw) == 0 and (t2 - t1) % (max(1, L // 2) * gpw) == 0
            runs, R1, R2 = runs_of(n, L, t1, t2)
            assert R1 % gpw == 0 and (R2 - R1) % gpw == 0  # a wave's runs share a zone: wave-uniform run length
            flat = np.concatenate([np.arange(a, b) for a, b in runs]) if runs else np.zeros(0, int)
            assert np.array_equal(flat, np.arange(n)), (n, L, gpw, tail)  # every triple once, in order
            lens = np.array([b - a for a, b in runs])
            assert np.all(lens[:R1] == L) and np.all(lens[R1:R2] == max(1, L // 2))
            assert np.all(lens[R2:-1] == max(1, L // 4)) and 1 <= lens[-1] <= max(1, L // 4 if R2 < len(runs) else L)
            if tail == 0:
                assert t1 == t2 and n - t1 < L * gpw  # only the ragged end goes in short runs


def test_deal_is_a_partition_with_the_short_runs_last():
    n, L, gpw, grid = 199_168, 8, 2, 224
    t1, t2 = zones(n, L, gpw, 12)
    runs, R1, R2 = runs_of(n, L, t1, t2)
    per = deal(len(runs), grid, gpw)
    allr = np.sort(np.concatenate([np.asarray(p) for p in per]))
    assert np.array_equal(allr, np.arange(len(runs)))
    sizes = [sum(runs[r][1] - runs[r][0] for r in p) for p in per]
    assert max(sizes) - min(sizes) <= 2 * L * gpw  # a workgroup's share: one wave-load of full runs at most apart
    for b, p in enumerate(per):
        assert p == sorted(p) and p[0] == b * gpw  # rising: the zones of short runs come last
        lens = [runs[r][1] - runs[r][0] for r in p]
        assert all(x >= y for x, y in zip(lens[:-1], lens[1:]))  # never a longer run after a shorter one
        for a, c in zip(p[:-gpw:gpw], p[gpw::gpw]):
            assert c - a == grid * gpw  # consecutive wave-loads of the launch sit on different workgroups


def test_private_deltas_lose_nothing_and_one_workgroup_is_sequential():
    rng = np.random.default_rng(3)
    I, n, L, gpw = 60, 5_000, 8, 2
    rows = (rng.zipf(1.3, n) % I).astype(int)
    hot = np.zeros(I, bool)
    hot[np.argsort(-np.bincount(rows, minlength=I))[:12]] = True
    q0 = rng.normal(0, 1, I)
    lr = 0.01
    grads = lambda v, t: -lr * (0.3 * v + np.sin(t))  # depends on the value read: staleness would show
    # one workgroup: exactly sequential SGD over the triples in order
    seq = q0.astype(np.float64).copy()
    for t in range(n):
        seq[rows[t]] += grads(seq[rows[t]], t)
    one, _ = run_launch(q0, rows, grads, 1, gpw, L, 12, hot)
    assert np.allclose(one, seq, rtol=0, atol=1e-12)
    # many workgroups, any interleaving: the table is the start plus the sum of every triple's update
    const = lambda v, t: 1.0 + 0.0 * v
    for order in ("round-robin", "random", "one-by-one"):
        many, _ = run_launch(q0, rows, const, 16, gpw, L, 12, hot, order=order, seed=5)
        assert np.allclose(many - q0, np.bincount(rows, minlength=I).astype(float), rtol=0, atol=1e-9), order
    # a workgroup sees its own updates of a hot row: with ONE hot row touched by one workgroup only the reads are sequential
    rows2 = np.concatenate([np.full(16, 7), rng.integers(20, 40, n - 16)])  # the first wave-load (workgroup 0) hits row 7
    hot2 = np.zeros(I, bool)
    hot2[7] = True
    _, reads = run_launch(np.zeros(I), rows2, const, 16, gpw, L, 0, hot2, order="random", seed=1)
    assert np.array_equal(reads[:16], np.arange(16.0))
    # what a workgroup misses of the others' updates of a hot row is at most their updates of this launch
    rows3 = np.full(n, 5)
    hot3 = np.zeros(I, bool)
    hot3[5] = True
    _, reads = run_launch(np.zeros(I), rows3, const, 16, gpw, L, 12, hot3, order="random", seed=2)
    assert reads.min() == 0.0 and reads.max() <= n / 16 + 2 * L * gpw  # each workgroup counts only its own ~n / 16


@pytest.mark.parametrize("n,L,K", [(2000, 8, 40), (1100, 3, 40), (600, 1, 24)])
def test_two_half_stream_keeps_the_two_groups_of_a_wave_apart(n, L, K):
    """The stream tests/test_gpu_hotlds.py holds the two groups of one G = 32 wave to the sequential oracle with:
    the runs a wave-load deals to its two groups share no user and no item row (positive or negative), every zone of
    the launch is there, users are cut by run boundaries, and the samplers — uniform, and adaptive on a model that
    moves — can only pick from the user's own half."""
    s = two_half_stream(n, L, 12, K, 30, seed=n + L)
    users, pos, neg, hu, hi, runs = s["users"], s["pos"], s["neg"], s["half_of_user"], s["half_of_item"], s["runs"]
    t1, t2 = zones(n, L, 2, 12)
    assert 0 < t1 < t2 < n and runs == runs_of(n, L, t1, t2)[0]
    assert deal(len(runs), 1, 2) == [list(range(len(runs)))]  # one workgroup: wave-load k = runs 2k, 2k + 1
    for k in range(0, len(runs), 2):
        a = slice(*runs[k])
        assert np.all(hu[users[a]] == 0) and np.all(hi[pos[a]] == 0) and np.all(hi[neg[a]] == 0)
        if k + 1 < len(runs):
            b = slice(*runs[k + 1])
            assert np.all(hu[users[b]] == 1) and np.all(hi[pos[b]] == 1) and np.all(hi[neg[b]] == 1)
            assert not set(users[a]) & set(users[b])
            assert not (set(pos[a]) | set(neg[a])) & (set(pos[b]) | set(neg[b]))
    assert users.min() >= 1 and pos.min() >= 1 and neg.min() >= 1
    # users cut by run boundaries: a group's run starts with the user its previous run ended with
    assert any(users[runs[r - 2][1] - 1] == users[runs[r][0]] for r in range(2, len(runs)))
    indptr, indices, I = s["indptr"], s["indices"], s["I"]
    for u in range(1, s["U"]):
        seen = indices[indptr[u]:indptr[u + 1]]
        assert np.array_equal(np.sort(seen[hi[seen] != hu[u]]), np.flatnonzero(hi == 1 - hu[u]))
    uni = oracle.sample_uniform(indptr, indices, I, users, seed=11, offset=5)
    assert np.array_equal(hi[uni], hu[users])
    rng = np.random.default_rng(0)
    d = 32
    P = rng.normal(0, 0.1, (s["U"], d)).astype(np.float32)
    Q = rng.normal(0, 0.1, (I, d)).astype(np.float32)
    P[0], Q[0] = 0, 0
    QT, sigma = oracle.adaptive_stats(Q)
    picks = np.zeros(n, np.int32)
    oracle.train_stream_seq(P, Q, None, users, pos, picks, oracle.NEG_ADAPTIVE, 0.05, (0.01, 0.02, 0.03),
                            adaptive_p=0.05, sigma=sigma, order=oracle.adaptive_order(QT), indptr=indptr,
                            indices=indices, seed=11)
    assert picks.min() >= 1 and np.array_equal(hi[picks], hu[users])
