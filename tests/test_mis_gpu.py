"""cusp::graph::maximal_independent_set and mis_aggregate (csrc/mis.hip) on the MI355X, through the C-ABI, against
tests/mis_refs.py.  All integer work: every comparison is exact (array_equal).  The largest case is poisson 300x300.
"""
import ctypes

import numpy as np
import pytest

import mis_refs as M

pytestmark = pytest.mark.gpu
INVALID = 1
SEEDS = (0, 0x1234567)


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


def graphs():
    """name -> (n, Ap, Aj): the reference's eight graphs, a star, a non-symmetric pattern, the deck made symmetric, and a graph
    with isolated nodes and empty rows.  Built once."""
    if not graphs.cache:
        out = dict(M.reference_graphs())
        out["star of 1000 leaves"] = M.star(1000)
        out["non-symmetric"] = M.non_symmetric(777, np.random.default_rng(21))
        rng = np.random.default_rng(22)
        lens = M.deck_lengths(rng)
        out["deck made symmetric"] = M.symmetrised(*M.random_pattern(rng, lens, len(lens)))
        # a path of 40 nodes in which every fifth node is cut out: empty rows, rows holding the diagonal alone, pairs and triples
        rows = []
        for i in range(40):
            if i % 5 == 0:
                rows.append([] if i % 10 == 0 else [i])
            else:
                rows.append([j for j in (i - 1, i, i + 1) if 0 <= j < 40 and j % 5 != 0])
        out["isolated nodes and empty rows"] = M.csr_from_rows(rows)
        graphs.cache = out
    return graphs.cache


graphs.cache = None
NAMES = ["two components of two", "path of 4", "K6", "six isolated", "poisson 3x3", "poisson 13x17", "poisson 23x24", "poisson 105x107", "star of 1000 leaves",
         "non-symmetric", "deck made symmetric", "isolated nodes and empty rows"]
_want = {}


def wanted(kind, name, *args):
    """The reference's answer, computed once per (kind, graph, arguments)."""
    key = (kind, name, args)
    if key not in _want:
        n, Ap, Aj = graphs()[name]
        _want[key] = M.mis(n, Ap, Aj, *args) if kind == "mis" else M.mis_aggregate(n, Ap, Aj, *args)
    return _want[key]


# ---- the sweep kernel alone ---------------------------------------------------------------------------------------------------
def device_ringmax(cmi, torch, n, Ap, Aj, x):
    z = cmi.csr_ring_max(n, dev(Ap, torch), dev(Aj, torch), dev(x.view(np.int64), torch))
    return z.cpu().numpy().view(np.uint64)


def random_keys(rng, n):
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


def test_sweep_row_lengths_around_the_wave(cmi, torch_cuda):
    """The strength test's deck: rows of 0..8, 63, 64, 65, 129 and 1000 entries, empty rows; columns unsorted and repeated, every
    seventh row without its diagonal."""
    rng = np.random.default_rng(11)
    lens = M.deck_lengths(rng)
    n, Ap, Aj = M.random_pattern(rng, lens, len(lens))
    rows = M.csr_rows(Ap)
    assert (np.bincount(rows[Aj == rows], minlength=n) == 0)[lens > 0].any()        # rows that do not store their diagonal
    assert any(len(set(Aj[Ap[i]:Ap[i + 1]])) < lens[i] for i in range(n))          # a repeated column
    x = random_keys(rng, n)
    got, want = device_ringmax(cmi, torch_cuda, n, Ap, Aj, x), M.ringmax(Ap, Aj, x)
    assert np.array_equal(got, want)
    assert np.array_equal(want, M.ringmax_loop(Ap, Aj, x))
    # keys whose halves disagree about the order: a maximum taken on one 32-bit half alone is caught
    x = (rng.integers(0, 4, size=n, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 2**32, size=n, dtype=np.uint64)
    assert np.array_equal(device_ringmax(cmi, torch_cuda, n, Ap, Aj, x), M.ringmax(Ap, Aj, x))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sweep_row_counts_around_the_wave_and_the_workgroup(cmi, torch_cuda, n):
    rng = np.random.default_rng(100 + n)
    _, Ap, Aj = M.random_pattern(rng, rng.integers(0, 7, size=n), n)
    x = random_keys(rng, n)
    assert np.array_equal(device_ringmax(cmi, torch_cuda, n, Ap, Aj, x), M.ringmax(Ap, Aj, x))
    # a column outside the matrix contributes nothing (and is not an address)
    if len(Aj):
        bad = Aj.copy()
        bad[0], bad[-1] = n, -1
        keep = np.ones(len(Aj), bool)
        keep[[0, -1]] = False
        rows = M.csr_rows(Ap)
        want = np.array(x)
        np.maximum.at(want, rows[keep], x[bad[keep]])
        assert np.array_equal(device_ringmax(cmi, torch_cuda, n, Ap, bad, x), want)


# ---- MIS(k) -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mis_equals_the_reference(cmi, torch_cuda, name):
    n, Ap, Aj = graphs()[name]
    dAp, dAj = dev(Ap, torch_cuda), dev(Aj, torch_cuda)
    for k in (0, 1, 2, 3):
        for seed in SEEDS if k else SEEDS[:1]:
            stencil, size, rounds = cmi.maximal_independent_set((n, dAp, dAj), k=k, seed=seed)
            want, want_rounds = wanted("mis", name, k, seed)
            print(f"{name}: k {k} seed {seed:#x}: set {size} of {n}, rounds {rounds}")
            assert np.array_equal(stencil.cpu().numpy(), want), (name, k, seed)
            assert size == int(want.sum()) and rounds == want_rounds, (name, k, seed)
            assert stencil.dtype == torch_cuda.int32
    if name == "poisson 13x17":
        assert [wanted("mis", name, k, 0)[0].sum() for k in (1, 2)] == [88, 34]


def test_mis_through_a_matrix_object(cmi, torch_cuda):
    A = cmi.poisson5pt(13, 17, "csr", device="cuda")
    stencil, size, rounds = cmi.maximal_independent_set(A)
    assert (size, rounds) == (88, 3) and int(stencil.sum()) == 88
    agg, mis, count = cmi.mis_aggregate(A)
    assert count == 34 and int(mis.sum()) == 34 and int(agg.max()) == 33 and int(agg.min()) == 0


# ---- mis_aggregate ------------------------------------------------------------------------------------------------------------
def check_aggregate(cmi, torch, n, Ap, Aj, want, seed, what):
    agg, mis, count = cmi.mis_aggregate((n, dev(Ap, torch), dev(Aj, torch)), seed=seed)
    assert np.array_equal(agg.cpu().numpy(), want[0]), what
    assert np.array_equal(mis.cpu().numpy(), want[1]), what
    assert count == want[2], what
    return agg.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_mis_aggregate_equals_the_reference(cmi, torch_cuda, name):
    n, Ap, Aj = graphs()[name]
    for seed in SEEDS:
        got = check_aggregate(cmi, torch_cuda, n, Ap, Aj, wanted("aggregate", name, seed), seed, (name, seed))
    if name == "isolated nodes and empty rows":                 # the singleton path: nodes cut out of the path are in no aggregate
        assert (got[::5] == -1).all() and (got >= 0).sum() == 32
    if name == "six isolated":
        assert (got == -1).all()
    if name == "non-symmetric":
        # -1 here comes from ids with fewer than two members.  The other -1 rule (a final key whose top part is 0) is a guard that
        # these sweeps cannot trip: a node left the MIS(2) rounds only on seeing a set node within two steps of its own rows.
        n, Ap, Aj = graphs()[name]
        m = wanted("aggregate", name, 0)[1].astype(np.uint64)
        y = M.ringmax(Ap, Aj, (m << np.uint64(31)) | np.arange(n, dtype=np.uint64)) + (m << np.uint64(31))
        assert ((M.ringmax(Ap, Aj, y) >> np.uint64(31)) != 0).all() and (got == -1).any()


def test_mis_aggregate_poisson_300x300(cmi, torch_cuda):
    n, Ap, Aj = M.poisson5pt(300, 300)
    want = M.mis_aggregate(n, Ap, Aj)
    got = check_aggregate(cmi, torch_cuda, n, Ap, Aj, want, 0, "poisson 300x300")
    sizes = np.bincount(got)
    assert got.min() == 0 and sizes.min() >= 2 and len(sizes) == want[2]


# ---- refusals and memory ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_column", ["num_rows", -1])
def test_a_column_out_of_range_is_refused_with_the_outputs_untouched(cmi, torch_cuda, bad_column):
    torch = torch_cuda
    L = cmi.lib()
    n, Ap, Aj = M.poisson5pt(23, 24)
    Aj = Aj.copy()
    Aj[1500] = n if bad_column == "num_rows" else -1
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    a, b = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    size, rounds = ctypes.c_int64(-7), ctypes.c_int(-7)
    for k in (1, 2, 3):
        assert L.cmi_csr_maximal_independent_set(n, len(Aj), vp(dAp), vp(dAj), k, 0, vp(a), ctypes.byref(size), ctypes.byref(rounds), None) == INVALID
        assert b"column index" in L.cmi_last_error()
    count = ctypes.c_int64(-7)
    assert L.cmi_csr_mis_aggregate(n, len(Aj), vp(dAp), vp(dAj), 0, vp(a), vp(b), ctypes.byref(count), None) == INVALID
    torch.cuda.synchronize()
    assert (a == -7).all() and (b == -7).all() and count.value <= 0 and size.value <= 0
    with pytest.raises(cmi.CmiError) as err:
        cmi.maximal_independent_set((n, dAp, dAj), k=2)
    assert err.value.status == INVALID


def test_scratch_is_returned(cmi, torch_cuda):
    torch = torch_cuda
    n, Ap, Aj = M.poisson5pt(60, 60)
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    bad = dAj.clone()
    bad[7] = n
    x = dev(np.arange(n, dtype=np.int64), torch)
    z = torch.empty_like(x)

    def refused():
        with pytest.raises(cmi.CmiError):
            cmi.mis_aggregate((n, dAp, bad))

    for call in (lambda: cmi.maximal_independent_set((n, dAp, dAj), k=1),
                 lambda: cmi.maximal_independent_set((n, dAp, dAj), k=3),
                 lambda: cmi.maximal_independent_set((n, dAp, dAj), k=0),
                 lambda: cmi.mis_aggregate((n, dAp, dAj)),
                 refused,
                 lambda: cmi.csr_ring_max(n, dAp, dAj, x, z)):
        assert_memory_returns(cmi, torch, call)


# ---- the header layer on device_memory ----------------------------------------------------------------------------------------
def test_mis_device_layer_program(cmi, torch_cuda, tmp_path):
    """tests/mis/test_mis_device.cpp, once, in a child process under its own time limit: device_memory results of
    maximal_independent_set and mis_aggregate against host_memory's on the five formats, and the mis_aggregation hierarchy on
    poisson 100x100 against the host one with rho supplied."""
    import os
    import subprocess
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_mis_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-I{os.path.join(ROOT, 'tests', 'amg')}",
                        os.path.join(ROOT, "tests", "mis", "test_mis_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "4 tests, 0 failed" in r.stdout
