"""CPU tests (-m "not gpu") of evolution strength of connection and cusp::gallery::diffusion on host_memory:
tests/evolution/test_evolution_host.cpp built once plainly and once as a stand-alone program under the address and
undefined-behaviour sanitizers; the measure it computes on decks written here against tests/evolution_refs.py -- offsets and
columns identical, values bit for bit; the compile-time refusals."""
import os
import struct
import subprocess

import numpy as np
import pytest

import evolution_refs as E
from conftest import ROOT
from special_values import same_bits

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "evolution")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}"]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
TESTS = "16 tests, 0 failed"


def hex_bits(v):
    v = np.asarray(v)
    return " ".join(f"{int(b):x}" for b in v.view(np.uint64 if v.dtype == np.float64 else np.uint32))


def write_deck(path, n, Ap, Aj, Ax, B, rho, epsilon):
    dbl = lambda x: struct.pack("<d", float(x))[::-1].hex()  # noqa: E731
    with open(path, "w") as f:
        f.write(f"{n} {len(Aj)} {dbl(rho)} {dbl(epsilon)}\n")
        f.write(" ".join(map(str, Ap.tolist())) + "\n" + " ".join(map(str, Aj.tolist())) + "\n" + hex_bits(Ax) + "\n" + hex_bits(B) + "\n")


def parse_measures(text, dtype):
    """The program's output for a list of decks: (Sp, Sj, Sx) per deck, None where it printed `refused`."""
    lines = iter(text.strip().split("\n"))
    out = []
    for head in lines:
        if head == "refused":
            out.append(None)
            continue
        tag, n, kept = head.split()
        assert tag == "S"
        Sp = np.array(next(lines).split(), np.int32)
        ent = [next(lines).split() for _ in range(int(kept))]
        bits = np.array([int(e[1], 16) for e in ent], np.uint64)
        Sx = bits.view(np.float64) if dtype == np.float64 else bits.astype(np.uint32).view(np.float32)
        assert len(Sp) == int(n) + 1
        out.append((Sp, np.array([int(e[0]) for e in ent], np.int32), Sx))
    return out


def run_measures(program, tmp_path, dtype, decks, prefix=()):
    paths = []
    for k, d in enumerate(decks):
        paths.append(str(tmp_path / f"deck{k}.txt"))
        write_deck(paths[-1], *d)
    r = subprocess.run([*prefix, program, "--measure", "f64" if dtype == np.float64 else "f32", *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = parse_measures(r.stdout, dtype)
    assert len(got) == len(decks)
    return got


def compare_with_the_restatement(got, decks, names):
    for g, d, name in zip(got, decks, names):
        assert g is not None, f"{name}: refused"
        want = E.evolution_strength(*d)["S"]
        assert np.array_equal(g[0], want[0]), f"{name}: row offsets differ"
        assert np.array_equal(g[1], want[1]), f"{name}: column indices differ"
        same_bits(g[2], want[2], name)


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("evolution") / "test_evolution_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_evolution_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_evolution_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert TESTS in r.stdout


def test_evolution_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_evolution_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_evolution_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert TESTS in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    # and the measure of one deck with long rows and one with infinities among its values
    decks = E.decks(np.float64)
    names = ["arrow 70", "tridiagonal 130 with gaps"]
    compare_with_the_restatement(run_measures(str(exe), tmp_path, np.float64, [decks[k] for k in names]), [decks[k] for k in names], names)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_measure_equals_the_restatement_bit_for_bit(host_program, tmp_path, dtype):
    decks = E.decks(dtype)
    names = list(decks)
    got = run_measures(host_program, tmp_path, dtype, [decks[k] for k in names])
    compare_with_the_restatement(got, [decks[k] for k in names], names)
    assert sum(len(g[1]) for g in got) > 1000


def test_host_measure_refuses_nonconforming_patterns(host_program, tmp_path):
    bad = E.nonconforming()
    decks = [(n, Ap, Aj, np.ones(len(Aj)), np.ones(n), 1.5, 4.0) for n, Ap, Aj in bad.values()]
    assert run_measures(host_program, tmp_path, np.float64, decks) == [None] * len(bad)


@pytest.mark.parametrize("snippet,needle", [
    ("cusp::ell_matrix<int, double, cusp::host_memory> A, S; cusp::array1d<double, cusp::host_memory> B; cusp::precond::aggregation::evolution_strength_of_connection(A, S, B);",
     "csr and coo matrices of one format"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A; cusp::coo_matrix<int, double, cusp::host_memory> S; cusp::array1d<double, cusp::host_memory> B; "
     "cusp::precond::aggregation::evolution_strength_of_connection(A, S, B);", "csr and coo matrices of one format"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A; cusp::csr_matrix<int, double, cusp::device_memory> S; cusp::array1d<double, cusp::host_memory> B; "
     "cusp::precond::aggregation::evolution_strength_of_connection(A, S, B);", "one memory space"),
    ("cusp::csr_matrix<int, double, cusp::host_memory> A; cusp::gallery::diffusion<int>(A, 3, 3);", "FD or FE"),
])
def test_evolution_refused_at_compile_time(tmp_path, snippet, needle):
    src = tmp_path / "bad.cpp"
    src.write_text("#include <cusp/ell_matrix.h>\n#include <cusp/gallery/diffusion.h>\n#include <cusp/precond/aggregation/smoothed_aggregation.h>\n" f"int main() {{ {snippet} return 0; }}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode != 0
    assert needle in r.stderr, r.stderr[-2000:]


def test_the_measure_and_the_gallery_compile_in_both_spaces(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/dia_matrix.h>\n#include <cusp/ell_matrix.h>\n#include <cusp/hyb_matrix.h>\n#include <cusp/gallery/diffusion.h>\n"
                   "#include <cusp/gallery/stencil.h>\n#include <cusp/precond/aggregation/smoothed_aggregation.h>\n"
                   "template <typename S, typename V> void f() { cusp::csr_matrix<int, V, S> A, C; cusp::coo_matrix<int, V, S> Ac, Cc; cusp::array1d<V, S> B;\n"
                   "  cusp::gallery::diffusion<cusp::gallery::FE>(A, 4, 4); cusp::gallery::diffusion<cusp::gallery::FD>(Ac, 4, 4, 1e-3, 0.0);\n"
                   "  cusp::dia_matrix<int, V, S> d; cusp::ell_matrix<int, V, S> e; cusp::hyb_matrix<int, V, S> h;\n"
                   "  cusp::gallery::diffusion<cusp::gallery::FE>(d, 4, 4); cusp::gallery::diffusion<cusp::gallery::FE>(e, 4, 4); cusp::gallery::diffusion<cusp::gallery::FE>(h, 4, 4);\n"
                   "  cusp::precond::aggregation::evolution_strength_of_connection(A, C, B); cusp::precond::aggregation::evolution_strength_of_connection(Ac, Cc, B, 1.5, 2.0);\n"
                   "  cusp::precond::aggregation::smoothed_aggregation<int, V, S> M; M.evolution_strength = true; M.evolution_epsilon = 3.0; M.initialize(A);\n"
                   "  cusp::precond::aggregation::smoothed_aggregation<int, V, cusp::host_memory> H(M); }\n"
                   "int main() { f<cusp::host_memory, double>(); f<cusp::host_memory, float>(); f<cusp::device_memory, double>(); f<cusp::device_memory, float>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
