"""References for cusp::graph::breadth_first_search, pseudo_peripheral_vertex, symmetric_rcm, connected_components, the gather /
scatter through an index map and permutation_matrix::symmetric_permute, written from the contracts of
include/cusp_mi355x.h.  All integer work or data movement: every comparison made against these is exact.

The graph is the stored pattern of a square CSR matrix: every stored entry of row u is an edge u -> column whatever its value,
columns may repeat, rows may be unsorted, edges are directed (the search follows rows).  A column of -1 is skipped; any other
column outside [0, n) in a row the search reaches raises Refused, in a row it does not reach it is not looked at.  Row offsets
are clamped to [0, num_entries]; a decreasing pair is an empty row.

  bfs(n, Ap, Aj, src, mark_levels)   (labels int32, reached, depth).  Levels, or predecessors: -2 the source, -1 not reached,
                                     else THE SMALLEST-NUMBERED vertex of the previous level with an edge to the vertex.
                                     No entries at all: labels all -1, reached 0, depth -1.
  pseudo_peripheral(n, Ap, Aj, start)  (vertex, levels, searches): search from x; y = the last-level vertex of smallest row
                                     length, smallest index on ties; stop when the depth no longer grows, else x = y.
  symmetric_rcm(n, Ap, Aj, start)    (permutation, vertex): vertices ordered by (level, index), level -1 first;
                                     permutation[v] = the position of v.
  connected_components(n, Ap, Aj)    (count, components): searches from 0, then from the first unset vertex; a search numbers
                                     every vertex it reaches (again, if need be) and its source.
  symmetric_permute(Ai, Aj, Ax, p)   COO entries (p[row], p[column], value) sorted by (row, column), stably.

bfs_loop is the search as a plain loop over a queue; MUTANTS names one deliberately wrong variant per rule of this library's
own, and tests/test_graph_refs.py proves that a deck catches each.  Plain module: no fixtures, no GPU.
"""
import numpy as np

from mis_refs import csr_rows

MUTANTS = ("first_discoverer", "first_count_valences")
INT32_MAX = 2**31 - 1


class Refused(ValueError):
    """what the library answers with CMI_ERROR_INVALID_VALUE / cusp::invalid_input_exception"""


def clamped_offsets(Ap, nnz):
    Ap = np.clip(np.asarray(Ap, np.int64), 0, nnz)
    lo, hi = Ap[:-1], np.maximum(Ap[1:], Ap[:-1])
    return lo, hi


def row_entries(lo, hi, rows):
    """(row of each entry, position of each entry) for the rows given, in the order given"""
    lens = hi[rows] - lo[rows]
    total = int(lens.sum())
    first = np.repeat(lo[rows] - (np.cumsum(lens) - lens), lens)
    return np.repeat(rows, lens), first + np.arange(total)


# ---- breadth-first search -----------------------------------------------------------------------------------------------------
def bfs(n, Ap, Aj, src, mark_levels=True, mutant=None):
    if not 0 <= src < n:
        raise Refused("source outside [0, n)")
    Aj = np.asarray(Aj, np.int64)
    if len(Aj) == 0:
        return np.full(n, -1, np.int32), 0, -1
    lo, hi = clamped_offsets(Ap, len(Aj))
    level = np.full(n, -1, np.int64)
    pred = np.full(n, INT32_MAX, np.int64)
    level[src] = 0
    frontier = np.array([src], np.int64)
    d = 0
    while True:
        u, at = row_entries(lo, hi, frontier)
        j = Aj[at]
        keep = j != -1
        u, j = u[keep], j[keep]
        if ((j < 0) | (j >= n)).any():
            raise Refused("a column index lies outside [0, n)")
        new = level[j] == -1
        u, j = u[new], j[new]
        if len(j) == 0:
            break
        if mutant == "first_discoverer":                        # the reference's host loop: queue order decides
            found, where = np.unique(j, return_index=True)
            order = np.argsort(where, kind="stable")
            frontier = found[order]
            pred[frontier] = u[where[order]]
        else:
            np.minimum.at(pred, j, u)
            frontier = np.unique(j)                             # (the queue's order is not observable)
        d += 1
        level[frontier] = d
    if mark_levels:
        return level.astype(np.int32), int((level >= 0).sum()), d
    labels = np.where(level < 0, -1, pred)
    labels[src] = -2
    return labels.astype(np.int32), int((level >= 0).sum()), d


def bfs_loop(n, Ap, Aj, src, mark_levels=True):
    """The contract as the header states it: a loop over levels, over the vertices of a level, over their rows."""
    if not 0 <= src < n:
        raise Refused("source outside [0, n)")
    nnz = len(Aj)
    if nnz == 0:
        return np.full(n, -1, np.int32), 0, -1
    clamp = lambda p: min(max(int(p), 0), nnz)  # noqa: E731
    level, pred = [-1] * n, [INT32_MAX] * n
    level[src] = 0
    this, d = [src], 0
    while this:
        nxt = []
        for u in this:
            for jj in range(clamp(Ap[u]), clamp(Ap[u + 1])):
                j = int(Aj[jj])
                if j == -1:
                    continue
                if j < 0 or j >= n:
                    raise Refused("a column index lies outside [0, n)")
                if level[j] == -1:
                    level[j] = d + 1
                    nxt.append(j)
                if level[j] == d + 1:
                    pred[j] = min(pred[j], u)
        if nxt:
            d += 1
        this = nxt
    reached = sum(l >= 0 for l in level)
    if mark_levels:
        return np.array(level, np.int32), reached, d
    return np.array([-2 if i == src else (-1 if level[i] < 0 else pred[i]) for i in range(n)], np.int32), reached, d


# ---- pseudo-peripheral vertex, level ordering, components ---------------------------------------------------------------------
def pseudo_peripheral(n, Ap, Aj, start=0, mutant=None):
    lo, hi = clamped_offsets(Ap, len(Aj))
    lens = hi - lo
    x, delta, searches = start, 0, 0
    while True:
        levels, _, depth = bfs(n, Ap, Aj, x)
        searches += 1
        last = np.flatnonzero(levels == depth)
        valence = lens[:len(last)] if mutant == "first_count_valences" else lens[last]   # the mutant: the reference's gather
        y = int(last[np.argmin(valence)])                       # (argmin: the first of equals, and `last` ascends)
        if levels[y] <= delta:
            return y, levels, searches
        x, delta = y, int(levels[y])


def symmetric_rcm(n, Ap, Aj, start=0):
    vertex, levels, _ = pseudo_peripheral(n, Ap, Aj, start)
    order = np.lexsort((np.arange(n), levels))
    permutation = np.empty(n, np.int32)
    permutation[order] = np.arange(n, dtype=np.int32)
    return permutation, vertex


def connected_components(n, Ap, Aj):
    components = np.full(n, -1, np.int32)
    count, src = 0, 0
    while src < n:
        labels, _, _ = bfs(n, Ap, Aj, src)
        components[labels >= 0] = count
        components[src] = count                                 # the library's guard: a matrix without entries reaches nobody
        count += 1
        unset = np.flatnonzero(components == -1)
        if len(unset) == 0:
            break
        src = int(unset[0])
    return count, components


# ---- data movement ------------------------------------------------------------------------------------------------------------
def gather(map, x):
    return np.asarray(x)[np.asarray(map)]


def scatter(map, x, m, fill=0):
    out = np.full(m, fill, np.asarray(x).dtype)
    out[np.asarray(map)] = x
    return out


def symmetric_permute(Ai, Aj, Ax, p):
    p = np.asarray(p)
    ni, nj = p[np.asarray(Ai)], p[np.asarray(Aj)]
    order = np.lexsort((nj, ni))                                # stable: sort_by_row_and_column
    return ni[order].astype(np.int32), nj[order].astype(np.int32), np.asarray(Ax)[order]


# ---- measures and graphs --------------------------------------------------------------------------------------------------------
def bandwidth(n, Ap, Aj):
    return int(np.abs(csr_rows(Ap) - np.asarray(Aj)).max()) if len(Aj) else 0


def level_width_bound(levels):
    """An edge of a symmetric pattern joins equal or adjacent levels, and a level ordering numbers a level consecutively: no
    edge is longer than max over l of width[l] + width[l + 1], minus 1."""
    w = np.r_[np.bincount(levels[levels >= 0]), 0]
    return int((w[:-1] + w[1:]).max()) - 1


def permuted_pattern(n, Ap, Aj, p):
    """The pattern with vertex v renamed p[v]; columns ascending."""
    ni, nj, _ = symmetric_permute(csr_rows(Ap), Aj, np.zeros(len(Aj)), p)
    return n, np.r_[0, np.cumsum(np.bincount(ni, minlength=n))].astype(np.int32), nj


def shuffled(n, Ap, Aj, seed):
    return permuted_pattern(n, Ap, Aj, np.random.default_rng(seed).permutation(n).astype(np.int32))


def random_symmetric(n, per_row, seed):
    """About per_row entries per row, the diagonal among them; symmetric, columns ascending, no repeats."""
    rng = np.random.default_rng(seed)
    m = n * (per_row - 1) // 2
    i, j = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keys = np.unique(np.r_[i * n + j, j * n + i, np.arange(n) * (n + 1)])
    rows, cols = keys // n, keys % n
    return n, np.r_[0, np.cumsum(np.bincount(rows, minlength=n))].astype(np.int32), cols.astype(np.int32)


def path(n):
    return n, np.r_[0, np.cumsum([len([j for j in (i - 1, i + 1) if 0 <= j < n]) for i in range(n)])].astype(np.int32), \
        np.array([j for i in range(n) for j in (i - 1, i + 1) if 0 <= j < n], np.int32)
