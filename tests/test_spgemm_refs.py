"""CPU tests (-m "not gpu") of tests/spgemm_refs.py itself: the numpy restatement of the SpGEMM contract against exact
rational arithmetic, against scipy.sparse (structure only), against its own literal loop, and against the five
deliberately wrong variants -- each caught by the deck spgemm_refs.CAUGHT_BY names for it."""
import os
from fractions import Fraction

import numpy as np
import pytest

import spgemm_refs as R
from conftest import GOLDEN, coo_to_csr, read_mtx
from special_values import bits_differ, same_bits


def same_csr(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: row offsets differ"
    assert np.array_equal(got[1], want[1]), f"{what}: column indices differ"
    same_bits(got[2], want[2], what)


def differs(got, want):
    return (not np.array_equal(got[0], want[0])) or (not np.array_equal(got[1], want[1])) or bool(bits_differ(got[2], want[2]).any())


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_reference_equals_exact_arithmetic_on_representable_inputs(dtype):
    rng = np.random.default_rng(11)
    for trial in range(6):
        m, k, n = (int(v) for v in rng.integers(1, 14, size=3))
        deck = list(R.random_pair(rng, m, k, n, 0.4, 0.4, dtype))
        # small integers times powers of two: every product and partial sum is exact in f32 already
        for x in (5, 8):
            deck[x] = (rng.integers(-8, 9, size=len(deck[x])) * 2.0 ** rng.integers(-3, 4, size=len(deck[x]))).astype(dtype)
        Cp, Cj, Cx = R.spgemm(*deck)
        want = R.exact(*deck)
        assert len(Cj) == len(want)
        for i in range(m):
            cols = Cj[Cp[i]:Cp[i + 1]]
            assert np.all(np.diff(cols) > 0)
            for q in range(Cp[i], Cp[i + 1]):
                assert Fraction(float(Cx[q])) == want[(i, int(Cj[q]))], (trial, i, int(Cj[q]))


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_reference_structure_equals_scipy(dtype):
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(12)
    for trial in range(6):
        m, k, n = (int(v) for v in rng.integers(0, 40, size=3))
        deck = R.random_pair(rng, m, k, n, 0.2, 0.3, dtype)
        _, _, _, Ap, Aj, Ax, Bp, Bj, Bx = deck
        Cp, Cj, _ = R.spgemm(*deck)
        # pattern product with all-ones values: scipy sums duplicates and never meets a cancellation
        S = sp.csr_matrix((np.ones(len(Aj)), Aj, Ap), shape=(m, k)) @ sp.csr_matrix((np.ones(len(Bj)), Bj, Bp), shape=(k, n))
        S.sort_indices()
        assert np.array_equal(Cp, S.indptr) and np.array_equal(Cj, S.indices), trial


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_fast_reference_equals_literal_loop(dtype):
    rng = np.random.default_rng(13)
    for name, deck in R.decks(dtype).items():
        same_csr(R.spgemm(*deck), R.spgemm_loop(*deck), name)
        same_csr(R.spgemm(*deck, drop_zeros=True), R.spgemm_loop(*deck, drop_zeros=True), name + " without zeros")
    for trial in range(5):
        m, k, n = (int(v) for v in rng.integers(0, 25, size=3))
        deck = R.random_pair(rng, m, k, n, 0.3, 0.3, dtype)
        same_csr(R.spgemm(*deck), R.spgemm_loop(*deck), f"random {trial}")
        same_csr(R.spgemm(*deck, drop_zeros=True), R.spgemm_loop(*deck, drop_zeros=True), f"random {trial} without zeros")


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_deck_answers_are_the_ones_the_contract_states(dtype):
    D = R.decks(dtype)
    T = np.dtype(dtype).type
    big = T(2.0) ** (53 if dtype == np.float64 else 24)
    Cp, Cj, Cx = R.spgemm(*D["order"])
    assert list(Cp) == [0, 2, 4] and list(Cj) == [0, 1, 0, 1] and Cx[0] == big
    Cp, Cj, Cx = R.spgemm(*D["minus_zero"])
    assert list(Cp) == [0, 1, 2] and not np.signbit(Cx).any() and np.all(Cx == 0)
    Cp, Cj, Cx = R.spgemm(*D["fma"])
    assert list(Cp) == [0, 1] and Cx[0] == 0 and not np.signbit(Cx[0])
    Cp, Cj, Cx = R.spgemm(*D["cancel"])
    assert list(Cp) == [0, 2, 4] and list(Cx) == [0.0, 5.0, 0.0, 0.0]
    assert len(R.spgemm(*D["cancel"], drop_zeros=True)[1]) == 1
    Cp, Cj, Cx = R.spgemm(*D["inf_nan"])
    assert list(Cp) == [0, 1, 2, 4, 6] and np.isnan(Cx[0]) and np.isnan(Cx[1]) and np.isnan(Cx[2]) and Cx[3] == -1.0
    assert Cx[4] == np.inf and Cx[5] == -np.inf
    assert len(R.spgemm(*D["inf_nan"], drop_zeros=True)[1]) == 6   # a NaN does not compare equal to zero: kept


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_caught_by_its_deck(dtype, mutant):
    D = R.decks(dtype)
    deck = D[R.CAUGHT_BY[mutant]]
    assert differs(R.spgemm_loop(*deck, mutant=mutant), R.spgemm(*deck)), f"{mutant} slipped through {R.CAUGHT_BY[mutant]}"
    if mutant == "drop_zeros":
        assert differs(R.spgemm_loop(*D["fma"], mutant=mutant), R.spgemm(*D["fma"]))


def test_transpose_and_aggregation_helpers():
    rows, cols, I, J, V = read_mtx(os.path.join(GOLDEN, "5pt_10x10.mtx"))
    Ap, Aj, Ax = coo_to_csr(rows, I, J, V)
    Tp, Tj, Tx = R.transpose(rows, cols, Ap, Aj, Ax)
    assert np.array_equal(Tp, Ap) and np.array_equal(Tj, Aj) and np.array_equal(Tx, Ax)  # symmetric, sorted rows
    Pp, Pj, Px = R.aggregation_2x2(4, 4, np.float64)
    assert list(Pj) == [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3] and Pp[-1] == 16 and np.all(Px == 1)
