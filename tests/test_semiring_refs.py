"""CPU tests of tests/semiring_refs.py: the restated loops are exact arithmetic for plus / multiplies where nothing rounds and plain selection
for minimum / maximum where neither a NaN nor a zero occurs; the decks contain what they promise; every deliberately wrong loop is caught by
the deck named for it."""
from fractions import Fraction

import numpy as np
import pytest

import semiring_refs as R
import special_values as sv

TAGS = ("f64", "f32")
DT = {"f64": np.float64, "f32": np.float32}


def formats(M, Ax, width=None):
    """The matrix in every format: csr, coo, ell, hyb (split at `width`, default R.hyb_width), and dia where M has diagonals."""
    width = R.hyb_width(M) if width is None else width
    f = {"csr": (M.Ap, M.Aj, Ax), "coo": (M.rows, M.Ai, M.Aj, Ax), "hyb": (M.rows,) + R.csr_to_hyb(M.Ap, M.Aj, Ax, width)}
    if M.row_lengths().max() <= R.ELL_MAX_WIDTH:      # (irregular has a row of 5000 entries: its ELL form is irregular_short's)
        f["ell"] = (M.rows,) + R.csr_to_ell(M.Ap, M.Aj, Ax)
    if hasattr(M, "dia_offsets"):
        f["dia"] = (M.rows, M.cols, M.dia_pitch, M.dia_offsets, R.csr_to_dia(M.rows, M.cols, M.Ap, M.Aj, Ax, M.dia_offsets, M.dia_pitch))
    return f


LOOPS = {"csr": R.semiring_csr, "coo": R.semiring_coo, "ell": R.semiring_ell, "hyb": R.semiring_hyb, "dia": R.semiring_dia}


def run(fmt, operands, x, combine, reduce, **kw):
    return LOOPS[fmt](*operands, x, combine, reduce, **kw)


@pytest.mark.parametrize("tag", TAGS)
def test_plus_and_multiplies_are_exact_rational_arithmetic(tag):
    """Small integers: no operation rounds, so the loops must equal arithmetic on Fractions, for the four arithmetic pairs and both starts."""
    M = sv.matrices(DT[tag])["poisson100"]
    Ax, x, y0 = R.small_integers(M, DT[tag])
    arith = {"plus": lambda a, b: a + b, "multiplies": lambda a, b: a * b}
    for combine in arith:
        for reduce in arith:
            for start in ("y0", 3.0):
                got = R.semiring_csr(M.Ap, M.Aj, Ax, x, combine, reduce, y0=y0 if start == "y0" else None, init=0.0 if start == "y0" else start)
                for i in range(0, M.rows, 7):
                    s = Fraction(float(y0[i])) if start == "y0" else Fraction(start)
                    for e in range(M.Ap[i], M.Ap[i + 1]):
                        s = arith[reduce](s, arith[combine](Fraction(float(Ax[e])), Fraction(float(x[M.Aj[e]]))))
                    assert Fraction(float(got[i])) == s, (combine, reduce, start, i)


@pytest.mark.parametrize("tag", TAGS)
def test_minimum_and_maximum_are_plain_selection_without_nans_and_zeros(tag):
    M = sv.matrices(DT[tag])["irregular"]
    Ax, x, y0 = R.decks(M, DT[tag])["ordinary"]
    assert not np.isnan(np.r_[Ax, x, y0]).any() and (np.r_[Ax, x, y0] != 0).all()
    for combine, pick in (("project1st", Ax), ("project2nd", x[M.Aj])):
        for reduce, sel in (("minimum", min), ("maximum", max)):
            got = R.semiring_csr(M.Ap, M.Aj, Ax, x, combine, reduce, y0=y0)
            want = np.array([sel([y0[i], *pick[M.Ap[i]:M.Ap[i + 1]]]) for i in range(M.rows)], DT[tag])
            R.same_bits(got, want, f"{combine} {reduce}")
    got = R.semiring_csr(M.Ap, M.Aj, Ax, x, "minimum", "maximum", init=-np.inf)
    want = np.array([max([DT[tag](-np.inf), *np.minimum(Ax, x[M.Aj])[M.Ap[i]:M.Ap[i + 1]]]) for i in range(M.rows)], DT[tag])
    R.same_bits(got, want, "minimum maximum")


@pytest.mark.parametrize("tag", TAGS)
def test_decks_contain_what_they_promise(tag):
    T = DT[tag]
    M = sv.matrices(T)["irregular"]
    d = R.decks(M, T)
    # NaNs at the first, the middle and the last entry of some rows
    _, x, _ = d["nan_positions"]
    seen = set()
    for r, pos in R.nan_rows(M).items():
        s, e = int(M.Ap[r]), int(M.Ap[r + 1])
        assert np.isnan(x[M.Aj[(s, (s + e - 1) // 2, e - 1)[pos]]])
        seen.add(pos)
    assert seen == {0, 1, 2} and 0 < np.isnan(x).sum() < M.cols // 4
    # zero ties in both orders inside rows: +0 followed by -0 and -0 followed by +0
    _, x, y0 = d["zero_ties"]
    g = np.signbit(x[M.Aj])
    inside = np.ones(M.nnz - 1, bool)
    inside[M.Ap[1:-1][(M.Ap[1:-1] > 0) & (M.Ap[1:-1] < M.nnz)] - 1] = False
    assert (x == 0).all() and (inside & ~g[:-1] & g[1:]).sum() >= 50 and (inside & g[:-1] & ~g[1:]).sum() >= 50
    assert np.signbit(y0[y0 == 0]).any() and not np.signbit(y0[y0 == 0]).all()
    assert np.isinf(R.INITS[0]) and np.isinf(R.INITS[1]) and R.INITS[0] > 0 > R.INITS[1] and np.isnan(R.INITS[2])
    # stored zeros on in-range diagonals of the DIA form; ELL padding
    B = sv.matrices(T)["banded"]
    Ax = R.decks(B, T)["stored_zeros"][0]
    vals = R.csr_to_dia(B.rows, B.cols, B.Ap, B.Aj, Ax, B.dia_offsets, B.dia_pitch)
    zeros_in_range = sum(1 for dd, k in enumerate(B.dia_offsets) for i in range(B.rows) if 0 <= i + int(k) < B.cols and vals[dd * B.dia_pitch + i] == 0)
    assert zeros_in_range >= B.nnz // 4 and zeros_in_range == int((Ax == 0).sum())
    S = R.matrices(T)["irregular_short"]
    width, pitch, eAj, _ = R.csr_to_ell(S.Ap, S.Aj, R.decks(S, T)["ordinary"][0])
    assert (eAj.reshape(width, pitch)[:, :S.rows] == -1).sum() == width * S.rows - S.nnz > S.rows
    assert M.row_lengths().max() == 5000 and 0 < R.hyb_width(M) < 64      # HYB of `irregular`: a real split, the long row in the COO part
    assert R.hyb_width(B) == 6 and B.row_lengths().min() == 6 and B.row_lengths().max() == 8
    for m in (M, S, B):                                                   # ... and of every matrix the decks run on: both parts have entries
        ell, coo = R.hyb_parts(m)
        _, _, _, _, cAi, _, _ = R.csr_to_hyb(m.Ap, m.Aj, np.zeros(m.nnz, T), R.hyb_width(m))
        assert ell > 0 and coo == len(cAi) > 0 and ell + coo == m.nnz


@pytest.mark.parametrize("tag", TAGS)
def test_formats_agree_on_every_deck(tag):
    """The same chain per row in CSR, COO, ELL and HYB (and DIA on the banded matrix, whose in-range slots are all entries)."""
    T = DT[tag]
    for name in ("irregular", "irregular_short", "banded"):
        M = R.matrices(T)[name]
        for dname, (Ax, x, y0) in R.decks(M, T).items():
            f = formats(M, Ax)
            for combine, reduce in (("plus", "minimum"), ("multiplies", "plus"), ("project2nd", "maximum")):
                want = run("csr", f["csr"], x, combine, reduce, y0=y0)
                for fmt in f:
                    R.same_bits(run(fmt, f[fmt], x, combine, reduce, y0=y0), want, f"{name} {dname} {fmt} {combine} {reduce}")


def differs(a, b):
    return int(sv.bits_differ(a, b).sum())


# mutant -> (matrix, format, deck, combine, reduce, start): the deck meant for it
CAUGHT_BY = {
    "fmin_fmax": ("irregular", "csr", "nan_positions", "project2nd", "minimum", "y0"),
    "tie_keeps_first": ("irregular", "csr", "zero_ties", "project2nd", "minimum", "y0"),
    "reversed_chain": ("irregular", "coo", "nan_positions", "project2nd", "minimum", np.inf),
    "start_at_first_term": ("irregular", "csr", "ordinary", "plus", "maximum", np.inf),
    "ell_padding_takes_part": ("irregular_short", "ell", "ordinary", "plus", "minimum", "y0"),
    "dia_skips_stored_zeros": ("banded", "dia", "stored_zeros", "plus", "minimum", "y0"),
    "hyb_coo_reinitialises": ("irregular", "hyb", "ordinary", "multiplies", "plus", "y0"),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
@pytest.mark.parametrize("tag", TAGS)
def test_every_mutant_is_caught_by_its_deck(tag, mutant):
    name, fmt, dname, combine, reduce, start = CAUGHT_BY[mutant]
    T = DT[tag]
    M = R.matrices(T)[name]
    Ax, x, y0 = R.decks(M, T)[dname]
    operands = formats(M, Ax)[fmt]
    kw = {"y0": y0} if isinstance(start, str) else {"init": start}
    right = run(fmt, operands, x, combine, reduce, **kw)
    wrong = run(fmt, operands, x, combine, reduce, mutant=mutant, **kw)
    assert differs(right, wrong) >= 3, f"{mutant} is not caught by {name} {dname} ({combine}, {reduce})"


def test_the_mutant_table_is_complete():
    assert set(CAUGHT_BY) == set(R.MUTANTS) and len(R.PAIRS) == 24 and [R.OP_CODE[n] for n in R.COMBINES] == list(range(6))
