"""References for cusp::graph::maximal_independent_set and cusp::precond::aggregation::mis_aggregate, written
from the contract of include/cusp_mi355x.h.  All integer work: every comparison made against these is exact.

The graph is the stored pattern of a square CSR matrix: every stored entry is an edge whatever its value, columns may repeat
and rows may be unsorted, and a node always sees itself whether or not its diagonal is stored.

  rand31(n, seed)     r(i) = cusp::detail::random_hash(i, seed) >> 33 (splitmix64's output function): 31 bits.
  ringmax(Ap, Aj, x)  z[i] = max(x[i], max over row i of x[Aj[jj]]) on uint64 keys.
  mis(n, Ap, Aj, k)   MIS(k).  States: 1 undecided, 2 in the set, 0 out; all start at 1.  A round: key = state << 62 |
                      r(i) << 31 | i; k ring sweeps, each on the previous one's result; an undecided node whose final key
                      carries its own index becomes 2; then an undecided node whose final key's index names a node that is now
                      2 becomes 0; stop when nobody is undecided.  k = 0: every node, no sweep, 0 rounds.
                      Returns (stencil int32 0/1, rounds).
  mis_aggregate       mis = MIS(2); key (mis << 31) | i, one sweep, mis << 31 added (the boost: 2 for a set node, 1 for its
                      neighbours), a second sweep; enum = exclusive scan of mis; a node takes enum[index of its final key], or
                      -1 when the key's top part is 0 (no set node within two steps: a non-symmetric pattern only).  Ids with
                      fewer than two members (an isolated node is its own set node; on a non-symmetric pattern a set node may
                      lose even itself) are removed: their nodes get -1, the remaining ids are renumbered densely in order.
                      Returns (aggregates int32, mis int32, num_aggregates).

Each step exists twice: vectorised (numpy) and as a plain loop (`*_loop`); tests/test_mis_refs.py holds them equal.  MUTANTS
names one deliberately wrong variant per rule; the same file proves that a deck catches each.
Plain module: no fixtures, no GPU.
"""
import numpy as np

MUTANTS = ("keys_without_index", "no_boost", "singletons_kept", "no_self")
MASK31 = np.uint64(0x7FFFFFFF)
U = np.uint64


def csr_rows(Ap):
    return np.repeat(np.arange(len(Ap) - 1), np.diff(Ap))


def random_hash(i, seed):
    """cusp::detail::random_hash on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = U(seed) + (np.asarray(i, np.uint64) + U(1)) * U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def random_hash_loop(i, seed):
    m = (1 << 64) - 1
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def rand31(n, seed=0):
    return random_hash(np.arange(n, dtype=np.uint64), seed) >> U(33)


# ---- the sweep --------------------------------------------------------------------------------------------------------------
def ringmax(Ap, Aj, x, mutant=None):
    n = len(Ap) - 1
    z = np.zeros(n, np.uint64) if mutant == "no_self" else np.array(x, np.uint64)
    if len(Aj):
        np.maximum.at(z, csr_rows(Ap), np.asarray(x, np.uint64)[Aj])
    return z


def ringmax_loop(Ap, Aj, x, mutant=None):
    n = len(Ap) - 1
    z = [0] * n
    for i in range(n):
        best = 0 if mutant == "no_self" else int(x[i])
        for jj in range(int(Ap[i]), int(Ap[i + 1])):
            best = max(best, int(x[Aj[jj]]))
        z[i] = best
    return np.array(z, np.uint64)


# ---- MIS(k) -----------------------------------------------------------------------------------------------------------------
def mis_keys(state, r, mutant=None):
    idx = np.zeros(len(state), np.uint64) if mutant == "keys_without_index" else np.arange(len(state), dtype=np.uint64)
    return (state.astype(np.uint64) << U(62)) | (r << U(31)) | idx


def mis(n, Ap, Aj, k, seed=0, mutant=None, sweep=ringmax):
    if k == 0:
        return np.ones(n, np.int32), 0
    r = rand31(n, seed)
    state = np.ones(n, np.int64)
    own = np.arange(n, dtype=np.uint64)
    rounds = 0
    while (state == 1).any():
        assert rounds <= n, "the round loop did not end"
        z = mis_keys(state, r, mutant)
        for _ in range(k):
            z = sweep(Ap, Aj, z, mutant)
        idx = z & MASK31
        undecided = state == 1
        state[undecided & (idx == own)] = 2
        state[undecided & (state == 1) & (state[idx.astype(np.int64)] == 2)] = 0
        rounds += 1
    return (state == 2).astype(np.int32), rounds


def mis_loop(n, Ap, Aj, k, seed=0):
    if k == 0:
        return np.ones(n, np.int32), 0
    r = [random_hash_loop(i, seed) >> 33 for i in range(n)]
    state = [1] * n
    rounds = 0
    while any(s == 1 for s in state):
        z = [(state[i] << 62) | (r[i] << 31) | i for i in range(n)]
        for _ in range(k):
            z = [int(v) for v in ringmax_loop(Ap, Aj, z)]
        for i in range(n):
            if state[i] == 1 and (z[i] & 0x7FFFFFFF) == i:
                state[i] = 2
        for i in range(n):
            if state[i] == 1 and state[z[i] & 0x7FFFFFFF] == 2:
                state[i] = 0
        rounds += 1
    return np.array([int(s == 2) for s in state], np.int32), rounds


# ---- aggregation ------------------------------------------------------------------------------------------------------------
def mis_aggregate(n, Ap, Aj, seed=0, mutant=None, sweep=ringmax):
    m, _ = mis(n, Ap, Aj, 2, seed, mutant=mutant if mutant == "no_self" else None, sweep=sweep)
    if n == 0:
        return np.zeros(0, np.int32), m, 0
    flag = m.astype(np.uint64)
    y = sweep(Ap, Aj, (flag << U(31)) | np.arange(n, dtype=np.uint64), mutant)
    if mutant != "no_boost":
        y = y + (flag << U(31))
    z = sweep(Ap, Aj, y, mutant)
    enum = np.cumsum(m, dtype=np.int64) - m
    total = int(m.sum())
    agg = np.where((z >> U(31)) == 0, -1, enum[(z & MASK31).astype(np.int64)])
    members = np.bincount(agg[agg >= 0], minlength=total)
    keep = members >= (1 if mutant == "singletons_kept" else 2)
    new_id = np.cumsum(keep) - keep
    out = np.where(agg >= 0, np.where(keep[np.maximum(agg, 0)], new_id[np.maximum(agg, 0)], -1), -1) if total else np.full(n, -1)
    return out.astype(np.int32), m, int(keep.sum())


def mis_aggregate_loop(n, Ap, Aj, seed=0):
    m, _ = mis_loop(n, Ap, Aj, 2, seed)
    y = ringmax_loop(Ap, Aj, [(int(m[i]) << 31) | i for i in range(n)])
    y = [int(y[i]) + (int(m[i]) << 31) for i in range(n)]
    z = ringmax_loop(Ap, Aj, y)
    enum, total = [], 0
    for i in range(n):
        enum.append(total)
        total += int(m[i])
    agg = [-1 if int(z[i]) >> 31 == 0 else enum[int(z[i]) & 0x7FFFFFFF] for i in range(n)]
    members = [0] * total
    for a in agg:
        if a >= 0:
            members[a] += 1
    new_id, count = [], 0
    for a in range(total):
        new_id.append(count if members[a] >= 2 else -1)
        count += members[a] >= 2
    return np.array([-1 if a < 0 else new_id[a] for a in agg], np.int32), m, count


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def csr_from_rows(rows):
    Ap = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    Aj = np.array([j for r in rows for j in r], np.int32)
    return len(rows), Ap, Aj


def poisson5pt(nx, ny):
    """The pattern of cusp::gallery::poisson5pt(nx, ny): node x + nx * y; columns ascending."""
    rows = []
    for y in range(ny):
        for x in range(nx):
            i = x + nx * y
            rows.append([j for j, ok in ((i - nx, y > 0), (i - 1, x > 0), (i, True), (i + 1, x < nx - 1), (i + nx, y < ny - 1)) if ok])
    return csr_from_rows(rows)


def reference_graphs():
    """The graphs of the reference's MIS test, explicit zeros removed: name -> (n, Ap, Aj)."""
    K6 = [[j for j in range(6)] for _ in range(6)]
    out = {
        "two components of two": csr_from_rows([[0, 1], [0, 1], [2, 3], [2, 3]]),
        "path of 4": csr_from_rows([[0, 1], [0, 1, 2], [1, 2, 3], [2, 3]]),
        "K6": csr_from_rows(K6),
        "six isolated": csr_from_rows([[] for _ in range(6)]),
    }
    for nx, ny in ((3, 3), (13, 17), (23, 24), (105, 107)):
        out[f"poisson {nx}x{ny}"] = poisson5pt(nx, ny)
    return out


def square_pattern(n, Ap, Aj):
    """The pattern of (A + I)^2 as adjacency sets: node -> the nodes within two steps (itself included)."""
    one = [set([i]) | set(int(j) for j in Aj[Ap[i]:Ap[i + 1]]) for i in range(n)]
    return one, [set().union(*(one[j] for j in one[i])) for i in range(n)]


def symmetrised(n, Ap, Aj):
    rows = [set() for _ in range(n)]
    for i, j in zip(csr_rows(Ap), Aj):
        rows[i].add(int(j))
        rows[int(j)].add(int(i))
    return csr_from_rows([sorted(r) for r in rows])


def star(leaves):
    """Node 0 joined to `leaves` leaves: one row of leaves + 1 entries."""
    return csr_from_rows([list(range(leaves + 1))] + [[0, i] for i in range(1, leaves + 1)])


def non_symmetric(n, rng, extra=2):
    """Upper bidiagonal plus random extra entries: unsorted, a column may repeat, some rows without a diagonal."""
    rows = []
    for i in range(n):
        r = ([] if i % 5 == 2 else [i]) + ([i + 1] if i + 1 < n else []) + rng.integers(0, n, size=rng.integers(0, extra + 1)).tolist()
        rows.append([r[p] for p in rng.permutation(len(r))])
    return csr_from_rows(rows)


def deck_lengths(rng):
    """The strength test's deck of row lengths: around the wave, one long row, empty rows."""
    return np.r_[rng.integers(0, 9, size=130), [63, 64, 65, 0, 1000, 0, 0, 64, 65, 129], rng.integers(0, 9, size=70)]


def random_pattern(rng, lens, n_cols, diag=True):
    """Rows of the given lengths, columns unsorted and possibly repeated, the diagonal stored in most rows."""
    rows = []
    for i, l in enumerate(lens):
        cols = rng.integers(0, n_cols, size=l)
        if diag and l and i % 7 != 3:
            cols[rng.integers(0, l)] = i
        rows.append(cols.tolist())
    return csr_from_rows(rows)
