"""cusp::graph breadth_first_search, pseudo_peripheral_vertex, symmetric_rcm and the gather / scatter of permutation_matrix
(csrc/bfs.hip) on the MI355X, through the C-ABI, against tests/graph_refs.py.  All integer work or data movement: every
comparison is exact (array_equal).  The largest graph is poisson 300x300 (598 levels from a corner).
"""
import ctypes

import numpy as np
import pytest

import graph_refs as G
import mis_refs as M

pytestmark = pytest.mark.gpu
INVALID = 1
GUARD = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def assert_memory_returns(cmi, torch, call):
    """`call` leaves the device bytes held by the library where they were (its own results are dropped before the reading)."""
    L = cmi.lib()
    call()                                                     # warm-up: code objects and the runtime's pools are in place
    before = free_bytes(torch)
    p = ctypes.c_void_p()
    cmi.check(L.cmi_malloc(ctypes.byref(p), 1))
    held = free_bytes(torch)
    cmi.check(L.cmi_free(p))
    slack = max(before - held, abs(before - free_bytes(torch)))
    base = free_bytes(torch)
    call()
    assert abs(free_bytes(torch) - base) <= slack, "scratch still held after the call"


def irregular_rows():
    """Unsorted rows, duplicates, self-loops, -1 columns, empty rows; vertices 9 and 10 form a second component; 11 is alone."""
    return M.csr_from_rows([[3, 1, 1, 0], [-1, 2, 0], [2, 2, 1, -1], [0, 4], [], [6, 5, -1, 4], [5, 7, 7], [8, 6], [7, -1], [10, 9], [9], []])


def graphs():
    """name -> (n, Ap, Aj), built once"""
    if not graphs.cache:
        out = dict(M.reference_graphs())
        for leaves in (63, 64, 65, 1000):
            out[f"star of {leaves} leaves"] = M.star(leaves)
        out["random symmetric 3000"] = G.random_symmetric(3000, 8, 31)
        out["non-symmetric"] = M.non_symmetric(777, np.random.default_rng(21))
        out["irregular rows"] = irregular_rows()
        out["shuffled poisson 60x60"] = G.shuffled(*M.poisson5pt(60, 60), 2)
        a, b = M.poisson5pt(9, 7), G.random_symmetric(50, 4, 6)
        out["disconnected"] = (a[0] + b[0], np.r_[a[1], a[1][-1] + b[1][1:]].astype(np.int32), np.r_[a[2], b[2] + a[0]].astype(np.int32))
        graphs.cache = out
    return graphs.cache


graphs.cache = None
REFERENCE = ["two components of two", "path of 4", "K6", "six isolated", "poisson 3x3", "poisson 13x17", "poisson 23x24", "poisson 105x107"]
STARS = ["star of 63 leaves", "star of 64 leaves", "star of 65 leaves", "star of 1000 leaves"]
OTHERS = ["random symmetric 3000", "non-symmetric", "irregular rows", "shuffled poisson 60x60", "disconnected"]
_want = {}


def wanted(kind, name, *args):
    """The reference's answer, computed once per (kind, graph, arguments)."""
    key = (kind, name, args)
    if key not in _want:
        n, Ap, Aj = graphs()[name]
        _want[key] = getattr(G, kind)(n, Ap, Aj, *args)
    return _want[key]


def guarded(torch, n):
    """an int32 device array of n elements between two guards of GUARD elements"""
    whole = torch.full((n + 2 * GUARD,), -77, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole, n):
    return bool((whole[:GUARD] == -77).all()) and bool((whole[GUARD + n:] == -77).all())


def device_bfs(cmi, torch, n, dAp, dAj, src, mark_levels):
    """through the raw symbol, into a guarded array: (labels, reached, depth)"""
    whole, labels = guarded(torch, n)
    reached, depth = ctypes.c_int64(-7), ctypes.c_int(-7)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cmi.check(cmi.lib().cmi_csr_breadth_first_search(n, dAj.numel(), vp(dAp), vp(dAj) if dAj.numel() else None, src, int(mark_levels), vp(labels),
                                                     ctypes.byref(reached), ctypes.byref(depth), None))
    torch.cuda.synchronize()
    assert guards_intact(whole, n)
    return labels.cpu().numpy(), reached.value, depth.value


def check_search(cmi, torch, n, Ap, Aj, src, want_levels=None, want_preds=None):
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    want_levels = want_levels or G.bfs(n, Ap, Aj, src)
    want_preds = want_preds or G.bfs(n, Ap, Aj, src, mark_levels=False)
    for mark, want in ((True, want_levels), (False, want_preds)):
        got = device_bfs(cmi, torch, n, dAp, dAj, src, mark)
        assert np.array_equal(got[0], want[0]), (src, mark)
        assert got[1:] == want[1:], (src, mark, got[1:], want[1:])


# ---- the search ---------------------------------------------------------------------------------------------------------------
def test_paths_of_every_length_around_a_batch_of_levels(cmi, torch_cuda):
    """1 .. 2 K + 2 vertices, K levels per host read, from an end and from the middle: the search ends at every phase of a batch."""
    K = cmi.bfs_levels_per_read()
    assert K >= 1
    for n in range(1, 2 * K + 3):
        _, Ap, Aj = G.path(n)
        for src in sorted({0, n // 2, n - 1}):
            check_search(cmi, torch_cuda, n, Ap, Aj, src)
    _, Ap, Aj = G.path(2 * K + 2)
    levels, reached, depth = cmi.breadth_first_search(2 * K + 2, dev(Ap, torch_cuda), dev(Aj, torch_cuda), 0)
    assert np.array_equal(levels.cpu().numpy(), np.arange(2 * K + 2)) and (reached, depth) == (2 * K + 2, 2 * K + 1)


@pytest.mark.parametrize("name", STARS + REFERENCE + OTHERS)
def test_search_equals_the_reference(cmi, torch_cuda, name):
    n, Ap, Aj = graphs()[name]
    for src in sorted({0, n // 2, 1, n - 1}) if name in STARS else (0, n // 2):
        check_search(cmi, torch_cuda, n, Ap, Aj, src, wanted("bfs", name, src), wanted("bfs", name, src, False))
    if name == "irregular rows":
        assert np.array_equal(wanted("bfs", name, 0)[0], [0, 1, 2, 1, 2, -1, -1, -1, -1, -1, -1, -1])
        check_search(cmi, torch_cuda, n, Ap, Aj, 11)            # an isolated source in a matrix that has entries
        assert wanted("bfs", name, 11)[1:] == (1, 0)
        check_search(cmi, torch_cuda, n, Ap, Aj, 9)
    if name == "non-symmetric":                                 # edges that lead one way only: following them backwards is shorter
        assert not np.array_equal(wanted("bfs", name, n // 2)[0], G.bfs(*M.symmetrised(n, Ap, Aj), n // 2)[0])
        n, Ap, Aj = M.csr_from_rows([[1], [2], [3], []])        # ... and vertices reachable one way only
        check_search(cmi, torch_cuda, n, Ap, Aj, 2)
        assert np.array_equal(G.bfs(n, Ap, Aj, 2)[0], [-1, -1, 0, 1])


def test_explicit_zeros_are_edges(cmi, torch_cuda):
    A = cmi.poisson5pt(3, 3, "csr", device="cuda")
    A.values.zero_()
    labels, reached, depth = cmi.breadth_first_search(9, A.row_offsets, A.column_indices, 0)
    assert np.array_equal(labels.cpu().numpy(), [0, 1, 2, 1, 2, 3, 2, 3, 4]) and (reached, depth) == (9, 4)


def test_many_simultaneous_discoverers_twice_bit_for_bit(cmi, torch_cuda):
    name = "random symmetric 3000"
    n, Ap, Aj = graphs()[name]
    dAp, dAj = dev(Ap, torch_cuda), dev(Aj, torch_cuda)
    want = wanted("bfs", name, 5, False)
    assert want[2] <= 8 and want[1] > 2900                      # shallow: hundreds of discoverers per level
    runs = [device_bfs(cmi, torch_cuda, n, dAp, dAj, 5, False) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1:] == runs[1][1:]
    assert np.array_equal(runs[0][0], want[0])


def test_poisson_300x300_from_a_corner(cmi, torch_cuda):
    n, Ap, Aj = M.poisson5pt(300, 300)
    x, y = np.arange(n) % 300, np.arange(n) // 300
    levels, reached, depth = cmi.breadth_first_search(n, dev(Ap, torch_cuda), dev(Aj, torch_cuda), 0)
    assert np.array_equal(levels.cpu().numpy(), x + y) and (reached, depth) == (n, 598)
    preds, _, _ = cmi.breadth_first_search(n, dev(Ap, torch_cuda), dev(Aj, torch_cuda), 0, mark_levels=False)
    want = np.where(y > 0, np.arange(n) - 300, np.arange(n) - 1)   # the smaller of the two candidates lies one row down
    want[0] = -2
    assert np.array_equal(preds.cpu().numpy(), want)


def test_no_entries_and_one_vertex(cmi, torch_cuda):
    torch = torch_cuda
    for n in (1, 6, 300):
        Ap, Aj = np.zeros(n + 1, np.int32), np.zeros(0, np.int32)
        for mark in (True, False):
            got = device_bfs(cmi, torch, n, dev(Ap, torch), dev(Aj, torch), n - 1, mark)
            assert (got[0] == -1).all() and got[1:] == (0, -1)
        vertex, levels, searches = cmi.pseudo_peripheral_vertex(n, dev(Ap, torch), dev(Aj, torch), n - 1)
        assert (vertex, searches) == (0, 1) and (levels.cpu().numpy() == -1).all()
        p, vertex = cmi.symmetric_rcm(n, dev(Ap, torch), dev(Aj, torch))
        assert np.array_equal(p.cpu().numpy(), np.arange(n)) and vertex == 0


@pytest.mark.parametrize("bad_column", ["num_rows", -2, 2**31 - 1])
def test_a_column_out_of_range_is_refused_only_where_the_search_comes(cmi, torch_cuda, bad_column):
    torch = torch_cuda
    L = cmi.lib()
    bad = 4 if bad_column == "num_rows" else bad_column
    n, Ap, Aj = M.csr_from_rows([[1], [0, 2], [1, bad], [3]])     # from 0 the search reaches row 2; from 3 it stays in row 3
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for mark in (1, 0):
        whole, labels = guarded(torch, n)
        reached, depth = ctypes.c_int64(-7), ctypes.c_int(-7)
        assert L.cmi_csr_breadth_first_search(n, len(Aj), vp(dAp), vp(dAj), 0, mark, vp(labels), ctypes.byref(reached), ctypes.byref(depth), None) == INVALID
        assert b"column index" in L.cmi_last_error()
        torch.cuda.synchronize()
        assert (labels == -1).all() and guards_intact(whole, n) and (reached.value, depth.value) == (0, -1)
        got = device_bfs(cmi, torch, n, dAp, dAj, 3, mark)
        assert np.array_equal(got[0], [-1, -1, -1, 0 if mark else -2]) and got[1:] == (1, 0)
    whole, out = guarded(torch, n)
    vertex, searches = ctypes.c_int64(-7), ctypes.c_int(-7)
    assert L.cmi_csr_pseudo_peripheral_vertex(n, len(Aj), vp(dAp), vp(dAj), 0, vp(out), ctypes.byref(vertex), ctypes.byref(searches), None) == INVALID
    assert L.cmi_csr_symmetric_rcm(n, len(Aj), vp(dAp), vp(dAj), 0, vp(out), ctypes.byref(vertex), None) == INVALID
    torch.cuda.synchronize()
    assert (whole == -77).all() and vertex.value == -7
    with pytest.raises(cmi.CmiError) as err:
        cmi.breadth_first_search(n, dAp, dAj, 1)
    assert err.value.status == INVALID


# ---- pseudo-peripheral vertex and the level ordering ------------------------------------------------------------------------
def check_ordering(cmi, torch, name, start):
    n, Ap, Aj = graphs()[name]
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    L = cmi.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    want_vertex, want_levels, want_searches = wanted("pseudo_peripheral", name, start)
    whole, levels = guarded(torch, n)
    vertex, searches = ctypes.c_int64(-7), ctypes.c_int(-7)
    cmi.check(L.cmi_csr_pseudo_peripheral_vertex(n, len(Aj), vp(dAp), vp(dAj) if len(Aj) else None, start, vp(levels), ctypes.byref(vertex), ctypes.byref(searches), None))
    torch.cuda.synchronize()
    assert guards_intact(whole, n)
    assert (vertex.value, searches.value) == (want_vertex, want_searches), (name, start)
    assert np.array_equal(levels.cpu().numpy(), want_levels), (name, start)
    want_p, _ = wanted("symmetric_rcm", name, start)
    whole, p = guarded(torch, n)
    cmi.check(L.cmi_csr_symmetric_rcm(n, len(Aj), vp(dAp), vp(dAj) if len(Aj) else None, start, vp(p), ctypes.byref(vertex), None))
    torch.cuda.synchronize()
    assert guards_intact(whole, n) and vertex.value == want_vertex
    assert np.array_equal(p.cpu().numpy(), want_p), (name, start)
    return want_levels, p.cpu().numpy()


@pytest.mark.parametrize("name", REFERENCE + OTHERS)
def test_pseudo_peripheral_vertex_and_ordering_equal_the_reference(cmi, torch_cuda, name):
    n, Ap, Aj = graphs()[name]
    for start in (0, n // 3, n - 1) if name == "shuffled poisson 60x60" else (0,):
        levels, p = check_ordering(cmi, torch_cuda, name, start)
        if name in ("disconnected", "two components of two", "irregular rows"):
            unreached = np.flatnonzero(levels == -1)
            assert len(unreached) and np.array_equal(np.sort(p[unreached]), np.arange(len(unreached)))   # they come first
        symmetric = name not in ("non-symmetric", "irregular rows")
        if symmetric and (levels >= 0).all():
            band = G.bandwidth(*G.permuted_pattern(n, Ap, Aj, p))
            print(f"{name} from {start}: bandwidth {G.bandwidth(n, Ap, Aj)} -> {band}, bound {G.level_width_bound(levels)}")
            assert band <= G.level_width_bound(levels)
    if name == "shuffled poisson 60x60":
        v, lv, s = cmi.pseudo_peripheral_vertex(n, dev(Ap, torch_cuda), dev(Aj, torch_cuda))
        assert (v, s) == wanted("pseudo_peripheral", name, 0)[::2] and lv.dtype == torch_cuda.int32


# ---- gather and scatter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
def test_gather_and_scatter(cmi, torch_cuda, n):
    torch = torch_cuda
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.int32)
    m = n + 5
    pick = rng.integers(0, m, size=n).astype(np.int32)          # a gather map need not be a bijection
    for dtype in (np.int32, np.float32, np.float64):
        x = (rng.standard_normal(m) * 1000).astype(dtype)
        assert np.array_equal(cmi.gather(dev(pick, torch), dev(x, torch), m).cpu().numpy(), G.gather(pick, x))
        y = x[:n]
        got = cmi.scatter(dev(perm, torch), dev(y, torch), n)
        assert np.array_equal(got.cpu().numpy(), G.scatter(perm, y, n))
        assert np.array_equal(cmi.scatter(dev(perm, torch), cmi.gather(dev(perm, torch), dev(y, torch), n), n).cpu().numpy(), y)
        assert got.dtype == dev(y, torch).dtype


@pytest.mark.parametrize("kind", ["gather", "scatter"])
@pytest.mark.parametrize("bad", [-1, "m", 2**31 - 1])
def test_a_map_entry_out_of_range_is_refused_and_moves_nothing_outside(cmi, torch_cuda, kind, bad):
    torch = torch_cuda
    L = cmi.lib()
    n = m = 1000
    map = np.random.default_rng(3).permutation(n).astype(np.int32)
    map[[0, 517, 999]] = m if bad == "m" else bad
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for suffix, dtype in (("i32", torch.int32), ("f32", torch.float32), ("f64", torch.float64)):
        x = torch.arange(n, device="cuda").to(dtype)
        whole = torch.full((n + 2 * GUARD,), -77, dtype=dtype, device="cuda")
        out = whole[GUARD:GUARD + n]
        assert getattr(L, f"cmi_{kind}_{suffix}")(n, m, vp(dev(map, torch)), vp(x), vp(out), None) == INVALID
        assert b"map entry" in L.cmi_last_error()
        torch.cuda.synchronize()
        assert (whole[:GUARD] == -77).all() and (whole[GUARD + n:] == -77).all()
        good = np.flatnonzero((map >= 0) & (map < m))
        got, xs = out.cpu().numpy(), x.cpu().numpy()
        if kind == "gather":
            assert np.array_equal(got[good], xs[map[good]]) and (got[[0, 517, 999]] == -77).all()
        else:
            assert np.array_equal(got[map[good]], xs[good])
    with pytest.raises(cmi.CmiError):
        getattr(cmi, kind)(dev(map, torch), torch.zeros(n, device="cuda"), m)


# ---- memory -------------------------------------------------------------------------------------------------------------------
def test_scratch_is_returned(cmi, torch_cuda):
    torch = torch_cuda
    n, Ap, Aj = M.poisson5pt(60, 60)
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    bad = dAj.clone()
    bad[7] = n
    map = dev(np.arange(n, dtype=np.int32)[::-1], torch)
    x = torch.zeros(n, device="cuda")

    def refused():
        with pytest.raises(cmi.CmiError):
            cmi.symmetric_rcm(n, dAp, bad)

    for call in (lambda: cmi.breadth_first_search(n, dAp, dAj, 0),
                 lambda: cmi.breadth_first_search(n, dAp, dAj, 7, mark_levels=False),
                 lambda: cmi.pseudo_peripheral_vertex(n, dAp, dAj),
                 lambda: cmi.symmetric_rcm(n, dAp, dAj),
                 refused,
                 lambda: cmi.gather(map, x, n),
                 lambda: cmi.scatter(map, x, n)):
        assert_memory_returns(cmi, torch, call)


# ---- drawn patterns -----------------------------------------------------------------------------------------------------------
def test_drawn_patterns(cmi, torch_cuda):
    """30 patterns of up to 300 vertices with any of the irregularities: unsorted rows, repeats, self-loops, -1 columns, empty
    rows, several components, directed edges."""
    from hypothesis import given, settings, strategies as st, HealthCheck

    @st.composite
    def patterns(draw):
        n = draw(st.integers(1, 300))
        seed = draw(st.integers(0, 2**32 - 1))
        density = draw(st.sampled_from([0.0, 0.5, 1.0, 2.0, 6.0]))
        symmetric, skips, window = draw(st.booleans()), draw(st.booleans()), draw(st.sampled_from([3, 40, 300]))
        rng = np.random.default_rng(seed)
        rows = [[] for _ in range(n)]
        for i in range(n):
            for j in (i + rng.integers(-window, window + 1, size=rng.poisson(density))).tolist():
                if 0 <= j < n:
                    rows[i].append(j)
                    if symmetric:
                        rows[j].append(i)
        for i in range(n):
            if skips and rows[i] and rng.random() < 0.3:
                rows[i].append(-1)
            rows[i] = [rows[i][k] for k in rng.permutation(len(rows[i]))]
        return M.csr_from_rows(rows), draw(st.integers(0, n - 1))

    @settings(max_examples=30, deadline=None, derandomize=True, database=None, suppress_health_check=list(HealthCheck))
    @given(patterns())
    def run(case):
        (n, Ap, Aj), src = case
        torch = torch_cuda
        check_search(cmi, torch, n, Ap, Aj, src)
        dAp, dAj = dev(Ap, torch), dev(Aj, torch)
        want_vertex, want_levels, want_searches = G.pseudo_peripheral(n, Ap, Aj, src)
        vertex, levels, searches = cmi.pseudo_peripheral_vertex(n, dAp, dAj, src)
        assert (vertex, searches) == (want_vertex, want_searches) and np.array_equal(levels.cpu().numpy(), want_levels)
        p, vertex = cmi.symmetric_rcm(n, dAp, dAj, src)
        assert vertex == want_vertex and np.array_equal(p.cpu().numpy(), G.symmetric_rcm(n, Ap, Aj, src)[0])

    run()


# ---- the header layer on device_memory ----------------------------------------------------------------------------------------
def test_graph_device_layer_program(cmi, torch_cuda, tmp_path):
    """tests/graph/test_graph_device.cpp, once, in a child process under its own time limit: device_memory results of the graph
    headers against host_memory's on the five formats (symmetric_permute entry for entry, both vector products), the components
    of the small graphs, the overloads and the refusals."""
    import os
    import subprocess
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_graph_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", *(f"-I{os.path.join(ROOT, 'tests', d)}" for d in ("cpp", "amg", "mis")),
                        os.path.join(ROOT, "tests", "graph", "test_graph_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "4 tests, 0 failed" in r.stdout
