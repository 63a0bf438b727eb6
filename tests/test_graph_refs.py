"""CPU tests (-m "not gpu") of tests/graph_refs.py: the references of the graph algorithms against scipy, and the rules that are
this library's own pinned by mutants that must fail."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import graph_refs as G
import mis_refs as M


def as_scipy(n, Ap, Aj):
    return sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(n, n))


def decks():
    if not decks.cache:
        out = dict(M.reference_graphs())
        out["star of 65 leaves"] = M.star(65)
        out["non-symmetric"] = M.non_symmetric(300, np.random.default_rng(5))
        out["random symmetric 300"] = G.random_symmetric(300, 6, 3)
        out["shuffled poisson 40x40"] = G.shuffled(*M.poisson5pt(40, 40), 7)
        out["path of 9"] = G.path(9)
        decks.cache = out
    return decks.cache


decks.cache = None
NAMES = ["two components of two", "path of 4", "K6", "six isolated", "poisson 3x3", "poisson 13x17", "poisson 23x24", "poisson 105x107", "star of 65 leaves",
         "non-symmetric", "random symmetric 300", "shuffled poisson 40x40", "path of 9"]


@pytest.mark.parametrize("name", NAMES)
def test_levels_equal_scipys_shortest_paths(name):
    n, Ap, Aj = decks()[name]
    for src in (0, n // 2):
        levels, reached, depth = G.bfs(n, Ap, Aj, src)
        if len(Aj) == 0:
            assert (levels == -1).all() and (reached, depth) == (0, -1)
            continue
        dist = csgraph.shortest_path(as_scipy(n, Ap, Aj), unweighted=True, indices=src, directed=True)
        want = np.where(np.isinf(dist), -1, dist).astype(np.int32)
        assert np.array_equal(levels, want)
        assert reached == (want >= 0).sum() and depth == want.max()
        assert np.array_equal(G.bfs_loop(n, Ap, Aj, src)[0], levels)


@pytest.mark.parametrize("name", NAMES)
def test_every_predecessor_lies_one_level_up_has_the_edge_and_is_the_smallest(name):
    n, Ap, Aj = decks()[name]
    if len(Aj) == 0:
        return
    src = n // 3
    levels = G.bfs(n, Ap, Aj, src)[0]
    pred, reached, depth = G.bfs(n, Ap, Aj, src, mark_levels=False)
    assert np.array_equal(pred, G.bfs_loop(n, Ap, Aj, src, mark_levels=False)[0])
    assert pred[src] == -2 and np.array_equal(pred == -1, levels == -1)
    A = as_scipy(n, Ap, Aj).tocsc()
    for j in np.flatnonzero(pred >= 0):
        sources = A.indices[A.indptr[j]:A.indptr[j + 1]]         # the vertices with an edge to j
        up = sources[levels[sources] == levels[j] - 1]
        assert pred[j] == up.min()


def test_the_min_index_rule_differs_from_the_queue_rule():
    n, Ap, Aj = G.shuffled(*M.poisson5pt(100, 100), 1)
    ours = G.bfs(n, Ap, Aj, 0, mark_levels=False)[0]
    queue = G.bfs(n, Ap, Aj, 0, mark_levels=False, mutant="first_discoverer")[0]
    differ = int((ours != queue).sum())
    print("labels that differ:", differ, "of", n)
    assert differ > 1000
    assert np.array_equal(G.bfs(n, Ap, Aj, 0)[0], G.bfs(n, Ap, Aj, 0, mutant="first_discoverer")[0])   # the levels do not


def test_the_valence_rule_differs_from_the_reference_gather():
    n, Ap, Aj = G.random_symmetric(300, 6, 3)
    ours = [G.pseudo_peripheral(n, Ap, Aj, s)[0] for s in range(0, 300, 10)]
    theirs = [G.pseudo_peripheral(n, Ap, Aj, s, mutant="first_count_valences")[0] for s in range(0, 300, 10)]
    assert ours != theirs
    lens = np.diff(Ap)
    for s in (0, 10):
        y, levels, searches = G.pseudo_peripheral(n, Ap, Aj, s)
        last = np.flatnonzero(levels == levels.max())
        assert levels[y] == levels.max() and lens[y] == lens[last].min() and y == last[lens[last] == lens[y]][0] and searches >= 2


@pytest.mark.parametrize("name", NAMES)
def test_component_count_equals_scipys_on_symmetric_patterns(name):
    n, Ap, Aj = decks()[name]
    count, comp = G.connected_components(n, Ap, Aj)
    assert (comp >= 0).all() and comp.max() == count - 1
    if name != "non-symmetric":
        want, labels = csgraph.connected_components(as_scipy(n, Ap, Aj), directed=False)
        assert count == want
        assert len(set(zip(comp.tolist(), labels.tolist()))) == count   # the same partition


@pytest.mark.parametrize("name", NAMES)
def test_the_ordering_is_a_bijection_and_bounds_the_bandwidth(name):
    n, Ap, Aj = decks()[name]
    p, vertex = G.symmetric_rcm(n, Ap, Aj)
    assert np.array_equal(np.sort(p), np.arange(n))
    _, levels, _ = G.pseudo_peripheral(n, Ap, Aj)
    assert np.array_equal(np.argsort(p), np.lexsort((np.arange(n), levels)))
    if name != "non-symmetric" and (levels >= 0).all():        # symmetric and connected
        got = G.bandwidth(*G.permuted_pattern(n, Ap, Aj, p))
        assert got <= G.level_width_bound(levels), name


def test_shuffled_poisson_comes_back_to_a_band():
    n, Ap, Aj = G.shuffled(*M.poisson5pt(100, 100), 1)
    before = G.bandwidth(n, Ap, Aj)
    p, _ = G.symmetric_rcm(n, Ap, Aj)
    _, levels, searches = G.pseudo_peripheral(n, Ap, Aj)
    after = G.bandwidth(*G.permuted_pattern(n, Ap, Aj, p))
    print("bandwidth", before, "->", after, "bound", G.level_width_bound(levels), "searches", searches)
    assert before > 9000 and after <= G.level_width_bound(levels) <= 2 * 100


def test_symmetric_permute_equals_scipys():
    rng = np.random.default_rng(9)
    n, Ap, Aj = G.random_symmetric(200, 5, 4)                   # no duplicate entries
    Ai, Ax = M.csr_rows(Ap), rng.standard_normal(len(Aj))
    p = rng.permutation(n).astype(np.int32)
    ni, nj, nx = G.symmetric_permute(Ai, Aj, Ax, p)
    want = sp.coo_matrix((Ax, (p[Ai], p[Aj])), shape=(n, n)).tocsr()
    want.sort_indices()
    assert np.array_equal(nj, want.indices) and np.array_equal(nx, want.data)
    assert np.array_equal(np.r_[0, np.cumsum(np.bincount(ni, minlength=n))], want.indptr)
    x = rng.standard_normal(n)
    assert np.array_equal(G.scatter(p, G.gather(p, x), n), x) and np.array_equal(G.gather(p, G.scatter(p, x, n)), x)


def test_refusals_and_skipped_columns():
    n, Ap, Aj = M.csr_from_rows([[1, -1], [0, 2, 2], [1], [7]])   # row 3 is not reachable from 0
    assert np.array_equal(G.bfs(n, Ap, Aj, 0)[0], [0, 1, 2, -1])
    with pytest.raises(G.Refused):
        G.bfs(n, Ap, Aj, 3)
    with pytest.raises(G.Refused):
        G.bfs_loop(n, Ap, Aj, 3)
    with pytest.raises(G.Refused):
        G.bfs(n, Ap, Aj, 4)
