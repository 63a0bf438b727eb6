"""cmi_csr_gauss_seidel_colour_* and cusp::relaxation::gauss_seidel / sor on the MI355X (-m gpu), against the numpy restatements
of tests/gauss_seidel_refs.py (proved on the CPU by tests/test_gauss_seidel_refs.py), compared by bit pattern with same_bits;
then the C++ device layer's program.

A sweep here is what the class does: the refs module's colouring and schedule, one C-ABI call per colour, the scratch passed
only for the colours whose rows depend on one another (`OnDevice.sweep`).  A wave of the kernel owns 64 consecutive slots and a
group of G lanes serves a row, G = 1 .. 64 from num_entries / num_rows.  Which case reaches which G (asserted in
test_every_group_size_is_reached with a restatement of the host rule):

    G = 1   one_row         1 x 1, one entry                                        (a one-row colour)
    G = 2   colour_sizes    193 rows, colours of exactly 63, 64, 65 rows and 1 row  (around the 64-slot tile)
    G = 4   poisson5        5-point stencil on 37 x 41: colours of 759 and 758 rows (both fall off the tile)
    G = 8   poisson9        9-point stencil on 23 x 19: four colours
    G = 16  features        300 rows, symmetric pattern: a row of 3000 entries, empty rows, rows without a diagonal, a stored 0
                            and a stored -0 diagonal, a diagonal stored twice
    G = 32  random32        120 rows, symmetric pattern, about 24 entries per row
    G = 64  dense64         100 rows, symmetric pattern, about 45 entries per row
    and the patterns that are NOT symmetric: the reference's 5 x 5 matrix (G = 2) and random200 (G = 8)
"""
import os
import subprocess

import numpy as np
import pytest

import gauss_seidel_refs as G
import special_values as sv
from conftest import ROOT
from special_values import same_bits

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
DIRECTIONS = (G.FORWARD, G.BACKWARD, G.SYMMETRIC)
M5 = [[1, 1, 2, 0, 0], [3, 2, 0, 0, 5], [0, 0, 0.5, 0, 0], [0, 6, 7, 4, 0], [0, 8, 0, 0, 8]]
CASE_G = {"one_row": 1, "colour_sizes": 2, "poisson5": 4, "poisson9": 8, "features": 16, "random32": 32, "dense64": 64,
          "reference5": 2, "random200": 8}
SYMMETRIC_CASES = ["one_row", "colour_sizes", "poisson5", "poisson9", "features", "random32", "dense64"]
CONFLICT_CASES = ["reference5", "random200"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


def group_size(rows, nnz):
    """The host rule: the smallest power of two >= num_entries // num_rows, between 1 and 64."""
    mean, g = nnz // rows, 1
    while g < 64 and mean > g:
        g *= 2
    return g


# ------------------------------------------------------------------------------------------------
# structures: name -> per-row column lists (the diagonal included where the row has one)
# ------------------------------------------------------------------------------------------------
def _stencil(m, n, nine):
    rows = []
    for r in range(m * n):
        ix, iy = r % m, r // m
        cols = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx and dy and not nine) or not (0 <= ix + dx < m and 0 <= iy + dy < n):
                    continue
                cols.append(r + dy * m + dx)
        rows.append(cols)
    return rows


def _symmetric_random(n, pairs, seed):
    rng = np.random.default_rng(seed)
    adj = [set() for _ in range(n)]
    for i, j in rng.integers(0, n, size=(pairs, 2)):
        if i != j:
            adj[i].add(int(j))
            adj[j].add(int(i))
    return [sorted(a | {i}) for i, a in enumerate(adj)]


def _colour_sizes():
    """Rows 0..3 open colours 0..3 (row c holds rows 0..c-1); every later row holds rows 0..c-1 for the colour c it is meant to take
    and so takes it: sizes 63, 64, 65 and 1.  No row holds a column of its own colour."""
    want = [0, 1, 2, 3] + [0] * 62 + [1] * 63 + [2] * 64
    order = np.random.default_rng(3).permutation(len(want) - 4) + 4
    colour_of = np.array(want)
    colour_of[4:] = np.array(want[4:])[order - 4]
    return [list(range(c)) + [i] for i, c in enumerate(colour_of)], colour_of


def _features():
    n, long_row = 300, 7
    kind = np.arange(n) % 25
    empty = set(np.flatnonzero(kind == 4).tolist())
    adj = [set() for _ in range(n)]
    live = [i for i in range(n) if i not in empty]
    for a, b in zip(live, live[1:]):               # a chain through the non-empty rows
        adj[a].add(b)
        adj[b].add(a)
    for i in live:                                  # everybody holds the long row, the long row holds everybody
        if i != long_row:
            adj[i].add(long_row)
            adj[long_row].add(i)
    rows = []
    for i in range(n):
        if i in empty:
            rows.append([])
        elif i == long_row:
            others = sorted(adj[i])
            cols = (others * (3000 // len(others) + 1))[:2999]
            rows.append(cols[:1500] + [i] + cols[1500:])          # 3000 entries, the diagonal in the middle
        elif kind[i] == 9:
            rows.append(sorted(adj[i]))                           # no diagonal
        elif kind[i] == 24:
            rows.append([i] + sorted(adj[i]) + [i])               # the diagonal stored twice
        else:
            rows.append(sorted(adj[i] | {i}))
    return rows, kind


def _structure(name):
    if name == "one_row":
        return [[0]]
    if name == "colour_sizes":
        return _colour_sizes()[0]
    if name == "poisson5":
        return _stencil(37, 41, False)
    if name == "poisson9":
        return _stencil(23, 19, True)
    if name == "features":
        return _features()[0]
    if name == "random32":
        return _symmetric_random(120, 1440, 32)
    if name == "dense64":
        return _symmetric_random(100, 3000, 64)
    if name == "reference5":
        return [list(np.flatnonzero(r)) for r in np.array(M5)]
    if name == "random200":
        rng = np.random.default_rng(200)
        return [sorted(set(rng.integers(0, 200, size=8).tolist()) | {i}) for i in range(200)]
    raise KeyError(name)


class Case:
    """A matrix in T with its schedule, b, x and the three expected sweeps (made once, never modified)."""

    def __init__(self, name, dtype):
        rows = _structure(name)
        self.name, self.n = name, len(rows)
        self.Ap = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
        self.Aj = np.array([j for r in rows for j in r], np.int32)
        rng = np.random.default_rng(sum(map(ord, name)))
        if name == "reference5":
            self.Ax = np.array(M5, dtype)[np.array(M5) != 0]
            self.b, self.x = np.full(5, 5, dtype), np.full(5, -1, dtype)
        else:
            self.Ax = rng.standard_normal(len(self.Aj)).astype(dtype)
            on_diag = self.Aj == np.repeat(np.arange(self.n), np.diff(self.Ap))
            self.Ax[on_diag] = (4 + rng.random(int(on_diag.sum()))).astype(dtype)
            self.b, self.x = rng.standard_normal(self.n).astype(dtype), rng.standard_normal(self.n).astype(dtype)
        if name == "features":
            kind = _features()[1]
            for i in np.flatnonzero((kind == 14) | (kind == 19)):                 # a stored 0, a stored -0: the row is left alone
                jj = self.Ap[i] + int(np.flatnonzero(self.Aj[self.Ap[i]:self.Ap[i + 1]] == i)[0])
                self.Ax[jj] = 0.0 if kind[i] == 14 else -0.0
            for i in np.flatnonzero(kind == 24):                                   # stored twice: the first must not be used
                self.Ax[self.Ap[i]] = 1000.0
        self.gs = G.GaussSeidel(self.Ap, self.Aj, self.Ax)
        self._want = {}

    def want(self, direction):
        if direction not in self._want:
            self._want[direction] = self.gs(self.b, self.x, direction)
        return self._want[direction]


_cases = {}


def case(name, dtype):
    key = (name, np.dtype(dtype).name)
    if key not in _cases:
        _cases[key] = Case(name, dtype)
    return _cases[key]


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class OnDevice:
    """The matrix, the schedule and b on the device, and x between NaN guard elements."""

    GUARD = 8

    def __init__(self, cmi, torch, c, x=None, b=None, Ax=None):
        self.cmi, self.torch, self.c = cmi, torch, c
        self.Ax0, self.b0 = (c.Ax if Ax is None else Ax), (c.b if b is None else b)
        self.Ap, self.Aj, self.Ax, self.b, self.ordering = (dev(a, torch) for a in (c.Ap, c.Aj, self.Ax0, self.b0, c.gs.ordering))
        self.buf = torch.full((c.n + 2 * self.GUARD,), float("nan"), dtype=self.Ax.dtype, device="cuda")
        self.x = self.buf[self.GUARD:self.GUARD + c.n]
        self.x.copy_(dev(c.x if x is None else x, torch))
        longest = int(np.diff(c.gs.color_offsets).max()) if c.gs.num_colors else 0
        self.scratch = torch.full((longest + self.GUARD,), float("nan"), dtype=self.Ax.dtype, device="cuda")

    def colour(self, k, parked, stream=None):
        s0, s1 = int(self.c.gs.color_offsets[k]), int(self.c.gs.color_offsets[k + 1])
        self.cmi.csr_gauss_seidel_colour(self.c.n, self.Ap, self.Aj, self.Ax, self.b, self.x, self.ordering, s0, s1,
                                         scratch=self.scratch if parked else None, stream=stream)

    def sweep(self, direction, park_all=False, stream=None):
        """What the class does: the scratch only for the colours that need it (park_all: for every colour)."""
        gs = self.c.gs
        for d in {G.FORWARD: (0,), G.BACKWARD: (1,), G.SYMMETRIC: (0, 1)}[direction]:
            for k in (range(gs.num_colors) if d == 0 else range(gs.num_colors - 1, -1, -1)):
                self.colour(k, park_all or bool(gs.color_conflicts[k]), stream)
        return self.x.cpu().numpy()

    def check_untouched(self):
        """The guard elements around x and behind the scratch still hold NaN; b and the matrix arrays have their bits."""
        g, c = self.GUARD, self.c
        buf = self.buf.cpu().numpy()
        assert np.isnan(buf[:g]).all() and np.isnan(buf[-g:]).all(), "a guard element next to x was written"
        assert np.isnan(self.scratch.cpu().numpy()[-g:]).all(), "the scratch was written behind the colour's length"
        same_bits(self.b.cpu().numpy(), self.b0, "b is read only")
        same_bits(self.Ax.cpu().numpy(), self.Ax0, "Ax is read only")
        assert np.array_equal(self.Ap.cpu().numpy(), c.Ap) and np.array_equal(self.Aj.cpu().numpy(), c.Aj)
        assert np.array_equal(self.ordering.cpu().numpy(), c.gs.ordering)


def test_every_group_size_is_reached():
    reached = set()
    for name, g in CASE_G.items():
        c = case(name, np.float64)
        assert group_size(c.n, len(c.Aj)) == g, (name, c.n, len(c.Aj))
        reached.add(g)
    assert reached == {1, 2, 4, 8, 16, 32, 64}
    # what the cases are meant to hold
    assert np.diff(case("colour_sizes", np.float64).gs.color_offsets).tolist() == [63, 64, 65, 1]
    assert np.diff(case("poisson5", np.float64).gs.color_offsets).tolist() == [759, 758]
    assert case("poisson9", np.float64).gs.num_colors == 4
    assert np.diff(case("features", np.float64).Ap).max() == 3000 and (np.diff(case("features", np.float64).Ap) == 0).sum() == 12
    assert np.diff(case("one_row", np.float64).gs.color_offsets).tolist() == [1]
    for name in SYMMETRIC_CASES:
        assert not case(name, np.float64).gs.color_conflicts.any(), name
    for name in CONFLICT_CASES:
        assert case(name, np.float64).gs.color_conflicts.any(), name      # at least one colour whose rows depend on one another


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", SYMMETRIC_CASES)
def test_sweeps_bit_exact(cmi, torch_cuda, name, dtype):
    c = case(name, dtype)
    for direction in DIRECTIONS:
        d = OnDevice(cmi, torch_cuda, c)
        same_bits(d.sweep(direction), c.want(direction), f"{name} direction {direction}")
        d.check_untouched()
    d = OnDevice(cmi, torch_cuda, c)          # the two-launch form on colours that do not need it: the same bits
    same_bits(d.sweep(G.SYMMETRIC, park_all=True), c.want(G.SYMMETRIC), f"{name} parked")
    d.check_untouched()


def test_features_rows_are_left_alone(cmi, torch_cuda):
    """Empty rows, rows without a diagonal, a stored 0 and a stored -0 keep their x; the twice-stored diagonal uses the last."""
    c = case("features", np.float64)
    kind = _features()[1]
    got = OnDevice(cmi, torch_cuda, c).sweep(G.FORWARD)
    alone = np.isin(kind, (4, 9, 14, 19))
    same_bits(got[alone], c.x[alone], "rows without a usable diagonal")
    assert not np.array_equal(got[~alone], c.x[~alone])
    same_bits(got, c.want(G.FORWARD), "features")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("name", CONFLICT_CASES)
def test_patterns_that_are_not_symmetric(cmi, torch_cuda, name, dtype):
    """Colours whose rows depend on one another: as the class runs them (the scratch for the flagged colours) and with the scratch
    on every colour -- both the host loop's bits, because a conflicting column is the larger index, visited later."""
    c = case(name, dtype)
    assert c.gs.color_conflicts.any()
    for direction in DIRECTIONS:
        for park_all in (False, True):
            d = OnDevice(cmi, torch_cuda, c)
            same_bits(d.sweep(direction, park_all=park_all), c.want(direction), f"{name} direction {direction} park_all {park_all}")
            d.check_untouched()
    if name == "reference5":
        assert c.want(G.SYMMETRIC).tolist() == [-1.4375, -13.5625, 10.0, 4.09375, 14.1875]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_slot_ranges_inside_a_colour(cmi, torch_cuda, dtype):
    """A range that is part of a colour, starting and ending off the 64-slot tile: the rows outside it keep their bits."""
    c = case("poisson5", dtype)
    for parked in (False, True):
        for s0, s1 in ((5, 70), (64, 128), (700, 759), (759, 760), (1516, 1517)):
            d = OnDevice(cmi, torch_cuda, c)
            cmi.csr_gauss_seidel_colour(c.n, d.Ap, d.Aj, d.Ax, d.b, d.x, d.ordering, s0, s1, scratch=d.scratch if parked else None)
            want = G.relax_slots(c.Ap, c.Aj, c.Ax, c.b, c.x.copy(), c.gs.ordering, s0, s1, parked=parked)
            got = d.x.cpu().numpy()
            same_bits(got, want, f"slots [{s0}, {s1}) parked {parked}")
            outside = np.ones(c.n, bool)
            outside[c.gs.ordering[s0:s1]] = False
            same_bits(got[outside], c.x[outside], "rows outside the range")
            d.check_untouched()
            if parked:   # the scratch holds the range's values at its start and nothing behind them
                park = d.scratch.cpu().numpy()
                same_bits(park[:s1 - s0], want[c.gs.ordering[s0:s1]], "parked values")
                assert np.isnan(park[s1 - s0:]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_nan_in_x_on_the_first_colour(cmi, torch_cuda, dtype):
    """NaN in x on exactly the rows of colour 0: a FORWARD sweep overwrites them without ever forming diagonal * x[i], and colour 1
    then reads finite values only."""
    c = case("poisson5", dtype)
    x = c.x.copy()
    x[c.gs.ordering[:c.gs.color_offsets[1]]] = np.nan
    d = OnDevice(cmi, torch_cuda, c, x=x)
    got = d.sweep(G.FORWARD)
    assert np.isfinite(got).all()
    same_bits(got, c.gs(c.b, x, G.FORWARD), "NaN on colour 0")
    d.check_untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("deck", sv.DECKS)
def test_special_value_decks(cmi, torch_cuda, deck, dtype):
    """The decks of tests/special_values.py on its 100 x 100 stencil: the matrix values as they are (signed, subnormal, huge, zeros
    on some diagonals), the deck's x -- NaN / inf on the near-miss columns, -0, subnormals -- once as x and once as b."""
    M = sv.matrices(dtype)["poisson100"]
    Ax, x, y0 = sv.decks(M, dtype)[deck]
    c = Case.__new__(Case)
    c.name, c.n, c.Ap, c.Aj, c.Ax = deck, M.rows, M.Ap, M.Aj, Ax
    c.gs = G.GaussSeidel(M.Ap, M.Aj, Ax)
    for b, x0 in ((y0, x), (x, y0)):
        c.b, c.x = b, x0
        d = OnDevice(cmi, torch_cuda, c)
        got = d.sweep(G.FORWARD)
        with np.errstate(all="ignore"):
            same_bits(got, c.gs(b, x0, G.FORWARD), f"{deck} forward")
        d.check_untouched()


def test_non_default_stream(cmi, torch_cuda):
    torch = torch_cuda
    c = case("random200", np.float64)
    d = OnDevice(cmi, torch, c)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    d.sweep(G.FORWARD, stream=s)
    s.synchronize()
    same_bits(d.x.cpu().numpy(), c.want(G.FORWARD), "on a stream of its own")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("omega", [1.5, 1.0])
def test_sor_steps(cmi, torch_cuda, omega, dtype):
    """temp = x; sweep; x = (1 - omega) * temp + omega * x -- the class's three calls."""
    for name in ("poisson5", "random200"):
        c = case(name, dtype)
        for direction in DIRECTIONS:
            d = OnDevice(cmi, torch_cuda, c)
            temp = d.x.clone()
            d.sweep(direction)
            T = np.dtype(dtype).type
            cmi.blas_axpby(float(T(1) - T(omega)), temp, omega, d.x, d.x)
            same_bits(d.x.cpu().numpy(), G.Sor(c.Ap, c.Aj, c.Ax, omega, direction)(c.b, c.x), f"{name} sor {omega} direction {direction}")
            d.check_untouched()


def test_empty_range_and_refused_arguments(cmi, torch_cuda):
    c = case("poisson5", np.float64)
    d = OnDevice(cmi, torch_cuda, c)
    cmi.csr_gauss_seidel_colour(c.n, d.Ap, d.Aj, d.Ax, d.b, d.x, d.ordering, 7, 7)     # empty: nothing happens
    same_bits(d.x.cpu().numpy(), c.x, "an empty range")
    for bad in ((3, 2), (-1, 4), (0, c.n + 1)):
        with pytest.raises((cmi.CmiError, ValueError)):
            cmi.csr_gauss_seidel_colour(c.n, d.Ap, d.Aj, d.Ax, d.b, d.x, d.ordering, *bad)
    with pytest.raises(cmi.CmiError) as e:
        cmi.csr_gauss_seidel_colour(c.n, d.Ap, d.Aj, d.Ax, d.x, d.x, d.ordering, 0, 4)
    assert e.value.status == 1 and "overlaps" in str(e.value)
    with pytest.raises(cmi.CmiError) as e:
        cmi.csr_gauss_seidel_colour(c.n, d.Ap, d.Aj, d.Ax, d.b, d.x, d.ordering, 0, 4, scratch=d.x[8:])
    assert e.value.status == 1 and "scratch overlaps" in str(e.value)
    same_bits(d.x.cpu().numpy(), c.x, "nothing was written by a refused call")


def test_gauss_seidel_cpp_device_layer(cmi, tmp_path):
    """tests/gauss_seidel/test_gs_device.cpp: the reference's cases, the colourings, the classes against the host restatement bit for
    bit on symmetric and non-symmetric patterns, copies between the memory spaces, the thrown exceptions."""
    import test_gauss_seidel_host as H
    exe = tmp_path / "test_gs_device"
    r = subprocess.run(["g++", *H.CXXFLAGS, os.path.join(ROOT, "tests", "gauss_seidel", "test_gs_device.cpp"), "-o", str(exe), *H.LDFLAGS],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert H.HOST_TESTS in r.stdout
    H.sor_lines_match_the_refs(r.stdout, "device_memory")
