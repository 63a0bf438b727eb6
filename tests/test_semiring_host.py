"""CPU tests (-m "not gpu") of the named functors through cusp::multiply and cusp::generalized_spmv on host_memory:
tests/semiring/test_semiring_host.cpp built plain and as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (as
tests/test_lanczos_host.py builds its program).  The program lays the five formats out as tests/semiring_refs.py does and prints every case in
hexadecimal; the results must be the loops' bit for bit.

Also home of the deck file both semiring programs read (write_decks / cases / expected), which tests/test_semiring_gpu.py uses for the device
program."""
import os
import subprocess

import numpy as np
import pytest

import semiring_refs as R
import special_values as sv
from conftest import GOLDEN, ROOT, coo_to_csr, read_mtx
from test_eigen_host import CXXFLAGS, LDFLAGS

SRC = os.path.join(ROOT, "tests", "semiring")
HOST_TESTS = "3 tests, 0 failed"
DEVICE_TESTS = "6 tests, 0 failed"
FORMATS = ("csr", "coo", "ell", "dia", "hyb")
TAGS = {"f64": np.float64, "f32": np.float32}


def build(tmp_path, source, name, extra=()):
    exe = tmp_path / name
    r = subprocess.run(["g++", *CXXFLAGS, *extra, os.path.join(SRC, source), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


class Deck:
    """One matrix (CSR arrays, the diagonals of its DIA form, where HYB splits it), x, y0 and the cases run on it."""

    def __init__(self, name, tag, rows, cols, Ap, Aj, Ax, x, y0, offsets, dia_pitch, width, cases):
        self.name, self.tag, self.T = name, tag, TAGS[tag]
        self.rows, self.cols, self.Ap, self.Aj, self.Ax, self.x, self.y0 = rows, cols, Ap, Aj, Ax, x, y0
        self.offsets, self.dia_pitch, self.width, self.cases = np.asarray(offsets, np.int32), int(dia_pitch), int(width), cases

    def write(self, f):
        hexes = lambda a: " ".join(float(v).hex() for v in a)  # noqa: E731
        ints = lambda a: " ".join(str(int(v)) for v in a)      # noqa: E731
        f.write(f"{self.tag} {self.rows} {self.cols} {len(self.Aj)} {self.width} {len(self.offsets)} {self.dia_pitch}\n")
        f.write("\n".join((ints(self.Ap), ints(self.Aj), hexes(self.Ax), hexes(self.x), hexes(self.y0), ints(self.offsets), str(len(self.cases)))) + "\n")
        for fmt, combine, reduce, start in self.cases:
            f.write(f"{fmt} {combine} {reduce} {start if isinstance(start, str) else float(start).hex()}\n")

    def expected(self):
        """The loops' result of every case, in order (formats other than DIA share the CSR chain: tests/test_semiring_refs.py)."""
        vals = R.csr_to_dia(self.rows, self.cols, self.Ap, self.Aj, self.Ax, self.offsets, self.dia_pitch) if len(self.offsets) else None
        out, cache = [], {}
        for fmt, combine, reduce, start in self.cases:
            kw = {"y0": self.y0} if start == "y0" else {"init": start}
            key = (fmt.endswith("dia"), combine, reduce, str(start))
            if key not in cache:
                if key[0]:
                    cache[key] = R.semiring_dia(self.rows, self.cols, self.dia_pitch, self.offsets, vals, self.x, combine, reduce, **kw)
                else:
                    cache[key] = R.semiring_csr(self.Ap, self.Aj, self.Ax, self.x, combine, reduce, **kw)
            out.append(cache[key])
        return out


def decks():
    """5pt_10x10 with all 24 pairs from y0 and from a constant in the five formats and through generalized_spmv; the special-value decks on
    irregular_short (ELL padding) and banded (stored zeros on in-range diagonals; DIA and its CSR / ELL / COO / HYB conversions), HYB with a real
    split on both, with +-inf and NaN as constants."""
    out = []
    rows, cols, I, J, V = read_mtx(os.path.join(GOLDEN, "5pt_10x10.mtx"))
    for tag, T in TAGS.items():
        Ap, Aj, Ax = coo_to_csr(rows, I, J, V, T)
        rng = np.random.default_rng(3)
        x, y0 = rng.standard_normal(cols).astype(T), rng.standard_normal(rows).astype(T)
        x[[7, 33, 34, 61]] = [np.nan, 0.0, -0.0, np.inf]
        y0[[2, 50]] = [-0.0, np.inf]
        cases = [(fmt, c, r, start) for c, r in R.PAIRS for start in ("y0", 2.5) for fmt in FORMATS]
        cases += [("g:" + fmt, c, r, "y0") for c, r in R.PAIRS for fmt in FORMATS]
        out.append(Deck("5pt_10x10", tag, rows, cols, Ap, Aj, Ax, x, y0, [-10, -1, 0, 1, 10], 112, 3, cases))
        pairs = (("multiplies", "plus"), ("plus", "minimum"), ("project2nd", "maximum"), ("project1st", "minimum"), ("maximum", "multiplies"))
        for name, fmts in (("irregular_short", ("csr", "coo", "ell", "hyb")), ("banded", FORMATS)):
            M = R.matrices(T)[name]
            for k, (dname, (Ax, x, y0)) in enumerate(R.decks(M, T).items()):
                cases = [(fmt, c, r, start) for c, r in pairs for start in ("y0", R.INITS[k % 3]) for fmt in fmts]
                dia = (M.dia_offsets, M.dia_pitch) if hasattr(M, "dia_offsets") else ([], 0)
                assert min(R.hyb_parts(M)) > 0, name      # HYB with a real split: both parts have entries
                out.append(Deck(f"{name} {dname}", tag, M.rows, M.cols, M.Ap, M.Aj, Ax, x, y0, dia[0], dia[1], R.hyb_width(M), cases))
    return out


def write_decks(path, all_decks):
    with open(path, "w") as f:
        for d in all_decks:
            d.write(f)


def parse(stdout, all_decks):
    """One line per case -> per deck a list of arrays of the deck's type."""
    lines = [l for l in stdout.split("\n") if l.strip()]
    assert len(lines) == sum(len(d.cases) for d in all_decks), (len(lines), sum(len(d.cases) for d in all_decks))
    out, at = [], 0
    for d in all_decks:
        out.append([np.array([float.fromhex(v) for v in lines[at + k].split()]).astype(d.T) for k in range(len(d.cases))])
        at += len(d.cases)
    return out


def compare(got, all_decks, who):
    for d, results in zip(all_decks, got):
        for case, y, want in zip(d.cases, results, d.expected()):
            sv.same_bits(y, want, f"{who} {d.name} {d.tag} {case}")


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    return build(tmp_path_factory.mktemp("semiring"), "test_semiring_host.cpp", "test_semiring_host")


@pytest.fixture(scope="module")
def deck_file(tmp_path_factory):
    all_decks = decks()
    path = tmp_path_factory.mktemp("semiring_decks") / "decks.txt"
    write_decks(path, all_decks)
    return path, all_decks


def test_semiring_host_layer_program(host_program):
    r = subprocess.run([str(host_program)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert HOST_TESTS in r.stdout


def test_host_multiply_is_the_loops_bit_for_bit(host_program, deck_file):
    """cusp::multiply and generalized_spmv with the named functors on host_memory, five formats, against semiring_refs."""
    path, all_decks = deck_file
    r = subprocess.run([str(host_program), "decks", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    compare(parse(r.stdout, all_decks), all_decks, "host")


def test_semiring_host_layer_program_under_sanitizers(cmi, tmp_path, deck_file):
    """The same stand-alone program built with -fsanitize=address,undefined (host code only; leak checking off: the HIP runtime the library
    links keeps process-lifetime allocations): the unit tests and every deck, same bits."""
    exe = build(tmp_path, "test_semiring_host.cpp", "test_semiring_host_asan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert HOST_TESTS in r.stdout and "runtime error" not in r.stderr
    path, all_decks = deck_file
    r = subprocess.run([str(exe), "decks", str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
    compare(parse(r.stdout, all_decks), all_decks, "host under sanitizers")
