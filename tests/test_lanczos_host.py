"""CPU tests (-m "not gpu") of cusp::eigen::lanczos, cusp::blas::gemm and cusp::detail::tridiagonal_eigen on host_memory:
tests/lanczos/test_lanczos_host.cpp built plain and as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (exactly as
tests/test_lobpcg_host.py builds its program).

Solver cases (tests/lanczos_refs.py CASES; poisson5pt on non-square grids, whose extreme eigenvalues are simple), bars computed in double from
the returned pairs, lambda_max < 8 the operator's largest eigenvalue:
  (i)   every lambda within res + 64 eps_T lambda_max of an eigenvalue of the dense matrix, res = ||A e - lambda e|| / ||e||;
  (ii)  the values are the wanted extremes within min(cap, max(10 x the restatement's error, 64 eps_T 8)), cap = 1e-9 (double) / 1e-5 (float);
  (iii) with Full: max |E^T E - I| <= m eps_T;
  (iv)  converged as the restatement says; iterations <= 1.5 x the restatement's count and <= maxIter;
  (v)   eigVals.size() and eigVecs.num_cols are the found counts; the low end ascending, then the high end.
Observed with the restatement (the library's start vector): value errors <= 1.6e-11 in double (33 x 31, LA 4), <= 2.5e-7 in float (16 x 12)
and <= 2.9e-7 in float on 7 x 5; orthogonality <= 0.23 m eps; at most 160 steps."""
import os
import subprocess

import numpy as np
import pytest

import lanczos_refs as R
from conftest import ROOT
from test_eigen_host import CXXFLAGS, LDFLAGS
from test_lanczos_refs import check_tridiagonal, tridiagonal_decks

SRC = os.path.join(ROOT, "tests", "lanczos")
HOST_TESTS = "10 tests, 0 failed"
EXTRA_FORMATS = ("coo", "ell", "dia", "hyb", "operator")


def build(tmp_path, source, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, source), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def expected_rows(device=False):
    """(case, format) in the order the programs print them."""
    rows = []
    for (nx, ny), t, tol in R.TABLE:
        if device and (nx, ny) == (7, 5):
            continue
        rows += [((nx, ny, t, part, count, "Full", tol), "csr") for part, count in R.PARTS]
        if nx == 16:
            rows.append(((nx, ny, t, R.LA, 1, "None", tol), "csr"))
            rows += [((nx, ny, t, R.LA, 4, "Full", tol), fmt) for fmt in EXTRA_FORMATS]
    return rows


def parse_cases(stdout):
    """`case nx ny type part count reorth tol format run <run> iterations <n> converged <0|1> found <f> rows <N> values <%a ...> vectors <%a ...>`"""
    out = []
    for line in stdout.split("\n"):
        if not line.startswith("case "):
            continue
        f = line.split()
        found, rows = int(f[16]), int(f[18])
        values = np.array([float.fromhex(x) for x in f[20:20 + found]])
        assert f[20 + found] == "vectors"
        flat = np.array([float.fromhex(x) for x in f[21 + found:]])
        assert len(flat) == found * rows, line[:200]
        out.append({"case": (int(f[1]), int(f[2]), f[3], f[4], int(f[5]), f[6], float(f[7])), "format": f[8], "run": f[10], "iterations": int(f[12]),
                    "converged": f[14] == "1", "values": values, "vectors": flat.reshape(found, rows).T if found else np.zeros((rows, 0))})
    return out


def check_row(row):
    return R.check_pairs(row["case"], row["values"], row["vectors"], row["iterations"], row["converged"], what=f"{row['run']} {row['format']}")


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    return build(tmp_path_factory.mktemp("lanczos"), "test_lanczos_host.cpp", "test_lanczos_host")


def test_lanczos_host_layer_program(host_program):
    r = subprocess.run([str(host_program)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_lanczos_host_layer_program_under_sanitizers(cmi, tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP runtime the library
    links keeps process-lifetime allocations).  minIter = 1 with three wanted values is among its tests: no read past T_iter's values."""
    exe = build(tmp_path, "test_lanczos_host.cpp", "test_lanczos_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr
    r = subprocess.run([str(exe), "cases"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and len(parse_cases(r.stdout)) == len(expected_rows()), r.stderr[-4000:]


def test_host_solver_cases(host_program):
    """Every case of the table under bars (i)-(v) of this file's head."""
    r = subprocess.run([str(host_program), "cases"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = parse_cases(r.stdout)
    assert [(row["case"], row["format"]) for row in rows] == expected_rows() and all(row["run"] == "host" for row in rows)
    for row in rows:
        check_row(row)
    none = [row for row in rows if row["case"] == (16, 12, "f64", R.LA, 1, "None", 1e-10)]
    assert len(none) == 1 and none[0]["converged"] and none[0]["iterations"] == 55


def gemm_decks():
    """(T, m, n, k, lda, ldb, ldc, A, B, C): tight and padded pitches, k = 0, a deck of signed zeros, infinities, NaN and subnormals."""
    rng = np.random.default_rng(11)
    decks = []
    for T in (np.float64, np.float32):
        for m, n, k, pa, pb, pc in ((5, 3, 4, 0, 0, 0), (7, 9, 5, 1, 2, 3), (4, 2, 0, 0, 1, 2), (1, 1, 1, 0, 0, 0), (33, 17, 70, 31, 0, 5)):
            lda, ldb, ldc = m + pa, k + pb, m + pc
            A, B, C = (rng.standard_normal(ld * cols).astype(T) for ld, cols in ((lda, k), (ldb, n), (ldc, n)))
            decks.append((T, m, n, k, lda, ldb, ldc, A, B, C))
        tiny = np.finfo(T).smallest_subnormal
        special = np.array([-0.0, 0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 1.0, -1.0, np.finfo(T).max, np.finfo(T).tiny], T)
        m, n, k = 6, 4, len(special)
        A = np.concatenate([np.roll(special, j)[:m] for j in range(k)]).astype(T)
        B = np.concatenate([np.roll(special[::-1], 3 * c) for c in range(n)]).astype(T)
        decks.append((T, m, n, k, m, k, m, A, B, np.full(m * n, np.nan, T)))
    return decks


def write_gemm_decks(path, decks):
    with open(path, "w") as f:
        for T, m, n, k, lda, ldb, ldc, A, B, C in decks:
            f.write(f"{'f64' if T is np.float64 else 'f32'} {m} {n} {k} {lda} {ldb} {ldc} " + " ".join(float(x).hex() for x in np.r_[A, B, C]) + "\n")


def gemm_expected(deck):
    """All of C after the call: the product inside, what it held elsewhere."""
    T, m, n, k, lda, ldb, ldc, A, B, C = deck
    want = C.copy().reshape(n, ldc)
    want[:, :m] = R.gemm_ref(A.reshape(k, lda)[:, :m].T.copy(), B.reshape(n, ldb)[:, :k].T.copy()).T
    return want.reshape(-1)


def parse_hex_lines(stdout):
    return [np.array([float.fromhex(x) for x in line.split()]) for line in stdout.strip().split("\n")]


def test_host_gemm_is_gemm_ref_bit_for_bit(host_program, tmp_path):
    """cusp::blas::gemm on host_memory views with padded pitches: the bits of gemm_ref inside C, the padding of C and all of A and B untouched."""
    import special_values as sv
    decks = gemm_decks()
    path = tmp_path / "gemm.txt"
    write_gemm_decks(path, decks)
    r = subprocess.run([str(host_program), "gemm", str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = parse_hex_lines(r.stdout)
    assert len(lines) == len(decks)
    for got, deck in zip(lines, decks):
        sv.same_bits(got.astype(deck[0]), gemm_expected(deck), f"gemm {deck[1:7]}")


def test_tridiagonal_eigen_on_the_decks(host_program, tmp_path):
    """cusp::detail::tridiagonal_eigen on the decks of tests/test_lanczos_refs.py, within the same bars."""
    decks = tridiagonal_decks()
    path = tmp_path / "tridiag.txt"
    path.write_text("".join(f"{len(d)} " + " ".join(float(x).hex() for x in list(d) + list(e)) + "\n" for d, e in decks.values()))
    r = subprocess.run([str(host_program), "tridiag", str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(decks)
    for line, (name, (d, e)) in zip(lines, decks.items()):
        f = line.split()
        n = len(d)
        assert f[0] == "1" and len(f) == 1 + n + n * n, name
        got = np.array([float.fromhex(x) for x in f[1:]])
        check_tridiagonal(name, d, e, got[:n], got[n:].reshape(n, n).T)
