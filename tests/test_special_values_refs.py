"""CPU checks of tests/special_values.py (no GPU): the oracle and the plain Python loops agree bit for bit on every deck, every
deck meets its floor counts on the reference's own output, every mutant loop is caught by the deck meant for it in at least
50 rows, and same_bits tells what it must."""
import numpy as np
import pytest

import special_values as sv

SMALL = ("poisson100", "banded", "runs")          # matrices whose ELL form stays small
DIA = ("poisson100", "banded")                    # ... and whose DIA form does
TAGS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}
NAMES = ("irregular", "poisson100", "banded", "runs", "band")


def ref_csr(orc, M, deck, accumulate):
    Ax, x, y0 = deck
    return orc.spmv_csr(M.Ap, M.Aj, Ax, x, y0 if accumulate else None)


# ---- same_bits ----
@pytest.mark.parametrize("dtype", sv.DTYPES)
def test_same_bits(dtype):
    a = np.array([0.0, 1.0, np.nan, np.inf], dtype)
    sv.same_bits(a, a.copy())
    with pytest.raises(AssertionError, match="differ in their bits"):
        sv.same_bits(np.array([-0.0], dtype), np.array([0.0], dtype))
    with pytest.raises(AssertionError):
        sv.same_bits(np.array([np.finfo(dtype).smallest_subnormal], dtype), np.array([0.0], dtype))
    # NaNs of either sign and any payload are one value
    u = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    quiet = np.array([np.nan], dtype)
    other = (quiet.view(u) | u(1) << u(8 * quiet.itemsize - 1) | u(5)).view(dtype)
    assert np.isnan(other[0]) and other.view(u)[0] != quiet.view(u)[0]
    sv.same_bits(other, quiet)
    with pytest.raises(AssertionError):
        sv.same_bits(quiet, np.array([1.0], dtype))
    with pytest.raises(AssertionError):
        sv.same_bits(np.array([1.0], dtype), quiet)
    with pytest.raises(AssertionError, match="dtype"):
        sv.same_bits(np.zeros(3, np.float32), np.zeros(3, np.float64))
    with pytest.raises(AssertionError, match="shape"):
        sv.same_bits(np.zeros(3, dtype), np.zeros(4, dtype))


# ---- the matrices are what the decks and the GPU table assume ----
def test_matrix_structure():
    for tag in TAGS:
        Ms = sv.matrices(DT[tag])
        assert set(Ms) == set(NAMES)
        for M in Ms.values():
            assert M.rows <= 10000 and M.nnz <= 120000 and M.Ap[0] == 0 and M.Ap[-1] == M.nnz
    M = sv.matrices(np.float64)["runs"]
    lens = M.row_lengths()
    assert (M.rows, M.cols) == (2000, 2003)
    assert np.all(lens[np.arange(M.rows) % 97 == 0] == 0) and lens.max() < 125
    assert np.all((lens == 0) | ((lens >= 24) & (lens <= 60)))
    single = three = 0
    ends = {M.cols - 1: 0, M.cols - 2: 0, M.cols - 3: 0, M.cols - 4: 0}
    run_lengths = set()
    for i in range(M.rows):
        c = M.Aj[M.Ap[i]:M.Ap[i + 1]]
        assert np.all(np.diff(c) > 0)
        have = set(c.tolist())
        pieces = sv._pieces(c)
        run_lengths.update(m for _, m in pieces)
        single += any(m == 1 and int(c[k]) + 1 not in have and int(c[k]) - 1 not in have for k, m in pieces)
        three += any(m == 3 and int(c[k]) + 3 not in have for k, m in pieces)
        if len(c) and int(c[-1]) in ends:
            ends[int(c[-1])] += 1
    assert run_lengths == {1, 2, 3, 4}
    assert single >= 50 and three >= 50 and min(ends.values()) >= 5, (single, three, ends)
    # the over-fetched neighbours of the near-miss pieces belong to no row at all
    assert len(M.near_miss_rows) >= 50 and not np.isin(M.Aj, M.near_miss_cols).any()
    B = sv.matrices(np.float64)["band"]
    lens = B.row_lengths()
    assert (B.rows, B.cols) == (4096, 4096) and lens.min() >= 16 and lens.max() <= 40
    assert np.all(np.abs(B.Aj.astype(np.int64) - B.Ai) <= 1500)
    centre = np.clip(B.Ai.astype(np.int64) - 1024, 0, B.cols - 2048)
    outside = (B.Aj < centre) | (B.Aj >= centre + 2048)
    assert np.bincount(B.Ai[outside], minlength=B.rows).mean() >= 2


# ---- oracle == Python loops, every deck ----
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_loops(orc, name, tag, accumulate):
    M = sv.matrices(DT[tag])[name]
    for dname, deck in sv.decks(M, DT[tag]).items():
        Ax, x, y0 = deck
        what = f"{name} {dname} {tag} acc {accumulate}"
        want = ref_csr(orc, M, deck, accumulate)
        sv.same_bits(sv.loop_spmv_csr(M.Ap, M.Aj, Ax, x, y0, accumulate), want, "csr " + what)
        sv.same_bits(orc.spmv_coo(M.rows, M.Ai, M.Aj, Ax, x, y0 if accumulate else None), want, "coo oracle " + what)
        if name == "irregular":
            sv.same_bits(sv.loop_spmv_coo(M.rows, M.Ai, M.Aj, Ax, x, y0, accumulate), want, "coo " + what)
        if name in SMALL:
            width = int(M.row_lengths().max())
            pitch, eAj, eAx = orc.csr_to_ell(M.Ap, M.Aj, Ax, width)
            got = orc.spmv_ell(M.rows, width, pitch, eAj, eAx, x, y0 if accumulate else None)
            sv.same_bits(got, want, "ell oracle against csr oracle " + what)
            sv.same_bits(sv.loop_spmv_ell(M.rows, width, pitch, eAj, eAx, x, y0, accumulate), got, "ell " + what)
            for w in (0, 3, width):
                pitch, hAj, hAx, cAi, cAj, cAx = orc.csr_to_hyb(M.Ap, M.Aj, Ax, w)
                got = orc.spmv_hyb(M.rows, w, pitch, hAj, hAx, cAi, cAj, cAx, x, y0 if accumulate else None)
                sv.same_bits(got, want, f"hyb {w} oracle against csr oracle " + what)
                if w == 3:
                    sv.same_bits(sv.loop_spmv_hyb(M.rows, w, pitch, hAj, hAx, cAi, cAj, cAx, x, y0, accumulate), got, f"hyb {w} " + what)
        if name in DIA:
            pitch, off, vals = orc.csr_to_dia(M.rows, M.cols, M.Ap, M.Aj, Ax)
            got = orc.spmv_dia(M.rows, M.cols, pitch, off, vals, x, y0 if accumulate else None)
            sv.same_bits(sv.loop_spmv_dia(M.rows, M.cols, pitch, off, vals, x, y0, accumulate), got, "dia " + what)


# ---- every deck's stated floor, on the reference's output alone ----
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", NAMES)
def test_deck_floors(orc, name, tag):
    dtype = np.dtype(DT[tag])
    M = sv.matrices(dtype)[name]
    D = sv.decks(M, dtype)
    lens, fi = M.row_lengths(), np.finfo(dtype)
    J = sv.nan_columns(M)
    assert {0, M.cols - 1, M.cols - 2} <= set(J.tolist())
    if name == "runs":
        assert set(M.near_miss_cols.tolist()) <= set(J.tolist())
    in_J = np.bincount(M.Ai, weights=np.isin(M.Aj, J), minlength=M.rows) > 0
    next_to_J = np.bincount(M.Ai, weights=np.isin(M.Aj, np.r_[J - 1, J + 1]), minlength=M.rows) > 0

    Ax, x, y0 = D["nan_near_miss"]
    assert np.isnan(x[J]).all() and np.isfinite(np.delete(x, J)).all() and np.isfinite(Ax).all()
    for acc in (False, True):
        y = ref_csr(orc, M, D["nan_near_miss"], acc)
        assert np.array_equal(np.isnan(y), in_J)
        assert int((next_to_J & ~in_J & np.isfinite(y)).sum()) >= 50 and int(np.isnan(y).sum()) >= 50
    if name == "runs":   # the dedicated near-miss rows are among the finite ones
        assert np.isfinite(ref_csr(orc, M, D["nan_near_miss"], False)[M.near_miss_rows]).all()

    Ax, x, y0 = D["inf_near_miss"]
    assert np.isinf(x[J]).all() and (x[J] > 0).any() and (x[J] < 0).any()
    zero_times_inf = np.bincount(M.Ai, weights=(Ax == 0) & np.isinf(x[M.Aj]), minlength=M.rows) > 0
    y = ref_csr(orc, M, D["inf_near_miss"], False)
    assert int(zero_times_inf.sum()) >= 10 and np.isnan(y[zero_times_inf]).all()
    assert int((next_to_J & ~in_J & np.isfinite(y)).sum()) >= 50 and np.all(~np.isfinite(y) == in_J)

    Ax, x, y0 = D["signed_zeros"]
    with np.errstate(all="ignore"):
        prod = Ax * x[M.Aj]
    assert np.all(prod == 0)
    neg = np.bincount(M.Ai, weights=np.signbit(prod), minlength=M.rows)
    all_neg, all_pos, mixed = (lens > 0) & (neg == lens), (lens > 0) & (neg == 0), (neg > 0) & (neg < lens)
    assert min(int(all_neg.sum()), int(all_pos.sum()), int(mixed.sum())) >= 100
    kinds = [np.signbit(y0) & (y0 == 0), ~np.signbit(y0) & (y0 == 0), y0 == dtype.type(-1.5)]
    assert all(int(k.sum()) >= M.rows // 3 for k in kinds)
    y = ref_csr(orc, M, D["signed_zeros"], False)
    assert np.all(y == 0) and not np.signbit(y).any()                 # 0 + (-0) = +0
    ya = ref_csr(orc, M, D["signed_zeros"], True)
    assert np.signbit(ya[all_neg & kinds[0]]).all() and not np.signbit(ya[all_pos & kinds[0]]).any()
    assert int((all_neg & kinds[0]).sum()) >= 30
    sv.same_bits(ya[lens == 0], y0[lens == 0], "empty rows keep y0 with its sign")
    if (lens == 0).sum() >= 9:
        assert all((k & (lens == 0)).any() for k in kinds)

    Ax, x, y0 = D["subnormals"]
    with np.errstate(all="ignore"):
        prod = Ax * x[M.Aj]
    assert np.all((prod > 0) & (prod < fi.tiny))
    for acc in (False, True):
        y = ref_csr(orc, M, D["subnormals"], acc)
        sub = (y > 0) & (y < fi.tiny)
        assert int(sub.sum()) >= 200 and np.all(sub | (lens == 0) | (lens > 200))
        # every sum is exact, so any order gives the same value
        exact = np.bincount(M.Ai, weights=prod.astype(np.float64), minlength=M.rows) + (y0.astype(np.float64) if acc else 0)
        assert np.array_equal(y.astype(np.float64), exact)

    Ax, x, y0 = D["overflow_order"]
    for acc in (False, True):
        y = ref_csr(orc, M, D["overflow_order"], acc)
        assert int(((lens >= 4) & np.isposinf(y)).sum()) >= 200 and np.all(np.isposinf(y[lens >= 4]))
        assert np.isfinite(y[lens < 4]).all()


# ---- the decks can see a bug: every mutant differs from the reference in at least 50 rows ----
@pytest.mark.parametrize("tag", TAGS)
def test_mutants_are_caught(orc, tag):
    dtype = DT[tag]
    M = sv.matrices(dtype)["runs"]
    D = sv.decks(M, dtype)
    width = int(M.row_lengths().max())

    def rows_off(mutant, dname, fmt, accumulate=False):
        Ax, x, y0 = D[dname]
        if fmt == "csr":
            want = ref_csr(orc, M, D[dname], accumulate)
            got = sv.loop_spmv_csr(M.Ap, M.Aj, Ax, x, y0, accumulate, mutant=mutant)
            sv.same_bits(sv.loop_spmv_csr(M.Ap, M.Aj, Ax, x, y0, accumulate), want)   # (the loop itself is right)
        else:
            pitch, eAj, eAx = orc.csr_to_ell(M.Ap, M.Aj, Ax, width)
            want = orc.spmv_ell(M.rows, width, pitch, eAj, eAx, x, y0 if accumulate else None)
            got = sv.loop_spmv_ell(M.rows, width, pitch, eAj, eAx, x, y0, accumulate, mutant=mutant)
        return int(sv.bits_differ(got, want).sum())

    for fmt in ("csr", "ell"):
        assert rows_off("start_at_first_product", "signed_zeros", fmt) >= 50, fmt
        assert rows_off("zero_times_padding", "nan_near_miss", fmt) >= 50, fmt
        assert rows_off("zero_times_padding", "inf_near_miss", fmt) >= 50, fmt
        assert rows_off("pairwise", "overflow_order", fmt) >= 50, fmt
        assert rows_off("pairwise", "overflow_order", fmt, accumulate=True) >= 50, fmt
        assert rows_off("flush_subnormals", "subnormals", fmt) >= 50, fmt
    # and the decks a mutant is NOT meant for need not see it: the ordinary part of a deck is not special
    assert set(sv.MUTANTS) == {"start_at_first_product", "zero_times_padding", "pairwise", "flush_subnormals"}
