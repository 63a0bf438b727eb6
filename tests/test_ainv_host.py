"""CPU tests (-m "not gpu") of the AINV preconditioners (cusp/precond/ainv.h) on host_memory: tests/ainv/test_ainv_host.cpp built once plainly and
once as a stand-alone program under the address and undefined-behaviour sanitizers; the factors it dumps against tests/ainv_refs.py -- offsets
and columns identical, values bit for bit; the reference's example compiled unchanged against the header layer."""
import os
import subprocess

import numpy as np
import pytest

import ainv_refs as R
from conftest import ROOT
from special_values import same_bits

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "ainv")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")   # oracle/Makefile's default
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}"]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
TESTS = "18 tests, 0 failed"


def parse_dump(text, dtype):
    """{setting index: {name: (offsets, columns, values) | values}} from the program's --dump output"""
    lines = iter(text.strip().split("\n"))
    out, cur = {}, None
    bits = lambda words: (np.array([int(w, 16) for w in words], np.uint64).view(np.float64) if dtype == np.float64  # noqa: E731
                          else np.array([int(w, 16) for w in words], np.uint64).astype(np.uint32).view(np.float32))
    for head in lines:
        tag, *rest = head.split()
        if tag == "S":
            cur = out.setdefault(int(rest[0]), {})
        elif tag == "M":
            name, rows, entries = rest[0], int(rest[1]), int(rest[2])
            offsets = np.array(next(lines).split(), np.int32)
            ent = [next(lines).split() for _ in range(entries)]
            assert len(offsets) == rows + 1
            cur[name] = (offsets, np.array([int(e[0]) for e in ent], np.int32), bits([e[1] for e in ent]))
        else:
            assert tag == "D"
            cur[rest[0]] = bits(next(lines).split())
            assert len(cur[rest[0]]) == int(rest[1])
    return out


def compare_csr(got, want, name):
    assert np.array_equal(got[0], want[0]), f"{name}: row offsets differ"
    assert np.array_equal(got[1], want[1]), f"{name}: column indices differ"
    same_bits(got[2], want[2], name)


def compare_with_the_restatement(dump, dtype, settings):
    n, Ap, Aj, Ax = R.poisson5pt(33, 31, dtype)
    nn, Bp, Bj, Bx = R.nonsymmetric(7, 5, dtype)
    entries = 0
    for k in settings:
        s, d = R.SETTINGS[k], dump[k]
        f = R.factor("scaled", n, Ap, Aj, Ax, dtype, *s)
        compare_csr(d["scaled.w"], f["w"], f"scaled.w {s}")
        compare_csr(d["scaled.w_t"], f["w_t"], f"scaled.w_t {s}")
        f = R.factor("bridson", n, Ap, Aj, Ax, dtype, *s)
        compare_csr(d["bridson.w"], f["w"], f"bridson.w {s}")
        compare_csr(d["bridson.w_t"], f["w_t"], f"bridson.w_t {s}")
        same_bits(d["bridson.diagonals"], f["diagonals"], f"bridson.diagonals {s}")
        entries += len(f["w"][1])
        for tag, args in (("nonsym", (n, Ap, Aj, Ax)), ("nonsym7x5", (nn, Bp, Bj, Bx))):
            f = R.factor("nonsym", *args, dtype, *s)
            compare_csr(d[tag + ".z"], f["z"], f"{tag}.z {s}")
            compare_csr(d[tag + ".w_t"], f["w_t"], f"{tag}.w_t {s}")
            same_bits(d[tag + ".diagonals"], f["diagonals"], f"{tag}.diagonals {s}")
    return entries


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("ainv") / "test_ainv_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_ainv_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_ainv_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert TESTS in r.stdout


def test_ainv_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_ainv_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_ainv_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert TESTS in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    # and the factors of the setting that replaces entries at full rows
    r = subprocess.run([str(exe), "--dump", "f32"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    compare_with_the_restatement(parse_dump(r.stdout, np.float32), np.float32, [2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_factors_equal_the_restatement_bit_for_bit(host_program, dtype):
    r = subprocess.run([host_program, "--dump", "f64" if dtype == np.float64 else "f32"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    dump = parse_dump(r.stdout, dtype)
    assert sorted(dump) == list(range(len(R.SETTINGS)))
    assert compare_with_the_restatement(dump, dtype, range(len(R.SETTINGS))) > 5000


def test_reference_example_compiles_unchanged(cmi, tmp_path):
    """examples/Preconditioners/ainv.cu of the reference against this header layer, with the flags oracle/Makefile uses for its examples; compile
    and link only, into tmp_path."""
    src = os.path.join(REFERENCE, "examples", "Preconditioners", "ainv.cu")
    if not os.path.exists(src):
        pytest.skip("the reference tree is not present")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-x", "c++", f"-I{INC}", src, "-x", "none", "-o", str(tmp_path / "ainv"), f"-L{LIBD}", "-lcusp_mi355x",
                        f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_ainv_compiles_in_both_spaces_for_every_format(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/coo_matrix.h>\n#include <cusp/csr_matrix.h>\n#include <cusp/dia_matrix.h>\n#include <cusp/ell_matrix.h>\n#include <cusp/hyb_matrix.h>\n"
                   "#include <cusp/krylov/cg.h>\n#include <cusp/precond/ainv.h>\n"
                   "template <typename M> void g(const M &A) { typedef typename M::value_type V; typedef typename M::memory_space S; cusp::array1d<V, S> x(A.num_rows), y(A.num_rows);\n"
                   "  cusp::precond::scaled_bridson_ainv<V, S> a(A); cusp::precond::bridson_ainv<V, S> b(A, .1, 4); cusp::precond::nonsym_bridson_ainv<V, S> c(A, 0, -1, true, 2);\n"
                   "  a(x, y); b(x, y); c(x, y); cusp::monitor<V> m(x); cusp::krylov::cg(A, x, y, m, a); cusp::krylov::cg(A, x, y, m, b); cusp::krylov::cg(A, x, y, m, c);\n"
                   "  cusp::linear_operator<V, S> &op = b; (void)op; (void)a.w; (void)a.w_t; (void)b.diagonals; (void)c.z; (void)c.w_t; }\n"
                   "template <typename S, typename V> void f() { g(cusp::csr_matrix<int, V, S>()); g(cusp::coo_matrix<int, V, S>()); g(cusp::ell_matrix<int, V, S>());\n"
                   "  g(cusp::dia_matrix<int, V, S>()); g(cusp::hyb_matrix<int, V, S>()); }\n"
                   "int main() { f<cusp::host_memory, double>(); f<cusp::host_memory, float>(); f<cusp::device_memory, double>(); f<cusp::device_memory, float>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
