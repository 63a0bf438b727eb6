"""CPU tests (-m "not gpu") of tests/mis_refs.py, the references for cusp::graph::maximal_independent_set and mis_aggregate:
the vectorised forms against the plain loops, the properties the reference's own test checks (independent and maximal in G and
G^2, counts, k = 0), the aggregation's invariants, the pinned values, and the mutants each rule must catch."""
import numpy as np
import pytest

import mis_refs as M

GRAPHS = M.reference_graphs()
SMALL = [name for name, g in GRAPHS.items() if g[0] <= 600]


def test_the_hash_is_the_librarys(cmi):
    L = cmi.lib()
    for seed in (0, 7, 2**63 + 5):
        got = M.random_hash(np.arange(50, dtype=np.uint64), seed)
        assert [int(v) for v in got] == [L.cmi_random_hash(i, seed) for i in range(50)] == [M.random_hash_loop(i, seed) for i in range(50)]
    assert int(M.rand31(1000).max()) < 2**31


@pytest.mark.parametrize("name", SMALL)
def test_vectorised_forms_equal_the_loops(name):
    n, Ap, Aj = GRAPHS[name]
    rng = np.random.default_rng(3)
    x = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    assert np.array_equal(M.ringmax(Ap, Aj, x), M.ringmax_loop(Ap, Aj, x))
    for seed in (0, 11):
        for k in (0, 1, 2, 3):
            a, b = M.mis(n, Ap, Aj, k, seed), M.mis_loop(n, Ap, Aj, k, seed)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (name, k, seed)
        a, b = M.mis_aggregate(n, Ap, Aj, seed), M.mis_aggregate_loop(n, Ap, Aj, seed)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (name, seed)


def test_loops_agree_on_unsorted_repeated_and_non_symmetric_patterns():
    rng = np.random.default_rng(4)
    for n, Ap, Aj in (M.non_symmetric(150, rng), M.random_pattern(rng, rng.integers(0, 9, size=120), 120), M.star(70)):
        x = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        assert np.array_equal(M.ringmax(Ap, Aj, x), M.ringmax_loop(Ap, Aj, x))
        for k in (1, 2, 3):
            a, b = M.mis(n, Ap, Aj, k, 5), M.mis_loop(n, Ap, Aj, k, 5)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        a, b = M.mis_aggregate(n, Ap, Aj, 5), M.mis_aggregate_loop(n, Ap, Aj, 5)
        assert np.array_equal(a[0], b[0]) and a[2] == b[2]


def independent_and_maximal(stencil, near):
    """No two set nodes see each other; every other node sees a set node (near[i]: what node i sees, itself included)."""
    chosen = set(np.flatnonzero(stencil).tolist())
    for i in range(len(near)):
        seen = near[i] & chosen
        if i in chosen:
            if seen != {i}:
                return False
        elif not seen:
            return False
    return True


@pytest.mark.parametrize("name", list(GRAPHS))
def test_mis_is_independent_and_maximal(name):
    n, Ap, Aj = GRAPHS[name]
    one, two = M.square_pattern(n, Ap, Aj)
    for seed in (0, 9):
        s0, r0 = M.mis(n, Ap, Aj, 0, seed)
        assert s0.tolist() == [1] * n and r0 == 0                # k = 0: every node
        s1, r1 = M.mis(n, Ap, Aj, 1, seed)
        s2, r2 = M.mis(n, Ap, Aj, 2, seed)
        assert independent_and_maximal(s1, one) and independent_and_maximal(s2, two), (name, seed)
        assert set(np.unique(s1)) <= {0, 1} and s1.dtype == np.int32
        assert 1 <= r1 <= n + 1 and 1 <= r2 <= n + 1
        if n > 9:
            assert s2.sum() < s1.sum() < n
    if name == "K6":
        assert M.mis(n, Ap, Aj, 1)[0].sum() == 1
    if name == "six isolated":
        assert M.mis(n, Ap, Aj, 1)[0].sum() == 6
    if name == "two components of two":
        assert M.mis(n, Ap, Aj, 1)[0].sum() == 2


def test_mis_on_a_host_built_pattern_and_its_square():
    """A symmetric pattern built here (a ring with chords, no stored diagonal) and the pattern of its square: MIS(1) of the square
    is a MIS(2) of the graph."""
    n = 61
    rows = [sorted({(i - 1) % n, (i + 1) % n, (i * 7) % n, next(j for j in range(n) if (j * 7) % n == i)} - {i}) for i in range(n)]
    n, Ap, Aj = M.csr_from_rows(rows)
    one, two = M.square_pattern(n, Ap, Aj)
    assert independent_and_maximal(M.mis(n, Ap, Aj, 1)[0], one) and independent_and_maximal(M.mis(n, Ap, Aj, 2)[0], two)
    _, Bp, Bj = M.csr_from_rows([sorted(t) for t in two])
    assert independent_and_maximal(M.mis(n, Bp, Bj, 1)[0], two)


@pytest.mark.parametrize("name", list(GRAPHS))
def test_aggregation_invariants(name):
    n, Ap, Aj = GRAPHS[name]
    agg, mis, count = M.mis_aggregate(n, Ap, Aj)
    assert np.array_equal(mis, M.mis(n, Ap, Aj, 2)[0])
    isolated = np.array([set(Aj[Ap[i]:Ap[i + 1]].tolist()) <= {i} for i in range(n)])
    assert (agg[isolated] == -1).all() and (agg[~isolated] >= 0).all()
    if count:
        sizes = np.bincount(agg[agg >= 0], minlength=count)
        assert len(sizes) == count and sizes.min() >= 2      # every id in [0, count) is used, by two nodes at least
        one, _ = M.square_pattern(n, Ap, Aj)
        roots = np.flatnonzero(mis & (agg >= 0))
        assert len(roots) == count and sorted(agg[roots].tolist()) == list(range(count))   # one set node in every aggregate
    else:
        assert name == "six isolated"


def test_pinned_values():
    for (nx, ny, k), (size, rounds, aggregates) in {(13, 17, 1): (88, 3, None), (13, 17, 2): (34, 3, 34), (100, 100, 2): (1422, 6, 1422)}.items():
        n, Ap, Aj = M.poisson5pt(nx, ny)
        s, r = M.mis(n, Ap, Aj, k)
        assert (int(s.sum()), r) == (size, rounds)
        if n < 1000:                                              # confirmed by the loop form
            sl, rl = M.mis_loop(n, Ap, Aj, k)
            assert np.array_equal(s, sl) and r == rl
        if aggregates is not None:
            agg, mis, count = M.mis_aggregate(n, Ap, Aj)
            assert count == aggregates
            if n == 10000:
                sizes = np.bincount(agg)
                assert agg.min() == 0 and (sizes.min(), sizes.max()) == (4, 13)
    n, Ap, Aj = M.poisson5pt(100, 100)
    agg, mis, count = M.mis_aggregate_loop(n, Ap, Aj)            # the 100x100 row confirmed by the loop form as well
    want = M.mis_aggregate(n, Ap, Aj)
    assert np.array_equal(agg, want[0]) and np.array_equal(mis, want[1]) and count == want[2] == 1422


def test_mutants_are_caught():
    assert set(M.MUTANTS) == {"keys_without_index", "no_boost", "singletons_kept", "no_self"}
    n, Ap, Aj = M.poisson5pt(13, 17)
    one, two = M.square_pattern(n, Ap, Aj)
    good = M.mis_aggregate(n, Ap, Aj)
    # keys without the index: a key names no node, so nobody ever finds its own index (or everybody finds node 0's)
    with pytest.raises(AssertionError):
        s, _ = M.mis(n, Ap, Aj, 1, mutant="keys_without_index")
        assert independent_and_maximal(s, one)
    # the boost makes a set node beat every key that is only NEAR a set node: a set node's direct neighbours join it, whatever the
    # index of another set node two steps away
    def neighbours_join_their_set_node(agg):
        return all(agg[j] == agg[r] for r in np.flatnonzero(good[1]) for j in Aj[Ap[r]:Ap[r + 1]])
    bad = M.mis_aggregate(n, Ap, Aj, mutant="no_boost")
    assert neighbours_join_their_set_node(good[0]) and not neighbours_join_their_set_node(bad[0])
    # singletons kept: isolated nodes keep an id
    g = M.csr_from_rows([[0, 1], [0, 1], [2], [], [4, 5], [4, 5]])
    kept = M.mis_aggregate(*g, mutant="singletons_kept")
    assert M.mis_aggregate(*g)[0].tolist() == [0, 0, -1, -1, 1, 1] and kept[2] == 4 and (kept[0] >= 0).all()
    # a node that does not see itself: without a stored diagonal its own key is lost
    ring = M.csr_from_rows([[(i - 1) % 9, (i + 1) % 9] for i in range(9)])
    x = np.arange(9, dtype=np.uint64)[::-1].copy()
    assert M.ringmax(ring[1], ring[2], x)[0] == 8 and M.ringmax(ring[1], ring[2], x, mutant="no_self")[0] == 7
    o, _ = M.square_pattern(*ring)
    assert independent_and_maximal(M.mis(*ring, 1)[0], o)
    with pytest.raises(AssertionError):
        s, _ = M.mis(*ring, 1, mutant="no_self")
        assert independent_and_maximal(s, o)
