"""CPU tests (-m "not gpu") of cusp::graph::breadth_first_search, pseudo_peripheral_vertex, symmetric_rcm, connected_components
and cusp::permutation_matrix on host_memory: tests/graph/test_graph_host.cpp built once plainly and once as a stand-alone
program under the address and undefined-behaviour sanitizers; what it prints for the five formats against tests/graph_refs.py,
exactly."""
import os
import subprocess

import numpy as np
import pytest

import graph_refs as G
import mis_refs as M
from conftest import ROOT, GOLDEN

INC = os.path.join(ROOT, "cusp-autotuned_amd", "include")
LIBD = os.path.join(ROOT, "cusp-autotuned_amd", "lib")
SRC = os.path.join(ROOT, "tests", "graph")
# the flags of tests/cpp/Makefile
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", f"-I{INC}",
            f"-I{os.path.join(ROOT, 'tests', 'cpp')}", f"-I{os.path.join(ROOT, 'tests', 'amg')}", f"-I{os.path.join(ROOT, 'tests', 'mis')}",
            f"-DGOLDEN_DIR=\"{GOLDEN}\""]
LDFLAGS = [f"-L{LIBD}", "-lcusp_mi355x", f"-Wl,-rpath,{LIBD}", "-Wl,-rpath,/opt/rocm/lib"]
TESTS = "3 tests, 0 failed"
FORMATS = ["coo", "csr", "ell", "dia", "hyb"]


@pytest.fixture(scope="module")
def host_program(cmi, tmp_path_factory):
    exe = tmp_path_factory.mktemp("graph") / "test_graph_host"
    r = subprocess.run(["g++", *CXXFLAGS, os.path.join(SRC, "test_graph_host.cpp"), "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def test_graph_host_layer_program(host_program):
    r = subprocess.run([host_program], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert TESTS in r.stdout


def test_graph_host_layer_program_under_sanitizers(cmi, tmp_path):
    # host code with its own main, built stand-alone with the sanitizers: their runtime is linked in, nothing is preloaded
    exe = tmp_path / "test_graph_host_san"
    r = subprocess.run(["g++", *CXXFLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(SRC, "test_graph_host.cpp"),
                        "-o", str(exe), *LDFLAGS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert TESTS in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def write_matrix(path, n, Ap, Aj):
    """the pattern with values 1, 2, 3, ... in storage order: the entries can be told apart"""
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {len(Aj)}\n")
        for e, (i, j) in enumerate(zip(M.csr_rows(Ap), Aj)):
            f.write(f"{i + 1} {j + 1} {e + 1}.0\n")


def parse_formats(text):
    """format -> {field: array or tuple of ints}"""
    out, cur = {}, None
    for line in text.strip().split("\n"):
        tag, *rest = line.split()
        if tag == "format":
            cur = out.setdefault(rest[0], {})
        elif tag == "values":
            cur[tag] = np.array(rest, np.float64)
        elif tag in ("search", "peripheral", "count"):
            cur[tag] = tuple(int(v) for v in rest)
        else:
            cur[tag] = np.array(rest, np.int32)
    return out


def decks():
    out = dict(M.reference_graphs())
    out["random symmetric 300"] = G.random_symmetric(300, 6, 3)
    out["shuffled poisson 20x20"] = G.shuffled(*M.poisson5pt(20, 20), 4)
    out["directed"] = M.csr_from_rows([[1], [2, 5], [3], [], [0], [4, 6], []])
    return out


@pytest.mark.parametrize("name", list(decks()))
def test_host_results_equal_the_references_in_all_five_formats(host_program, tmp_path, name):
    n, Ap, Aj = decks()[name]
    path = tmp_path / "matrix.mtx"
    write_matrix(path, n, Ap, Aj)
    for src, start in ((0, 0), (n // 2, n // 3)):
        r = subprocess.run([host_program, "--print", str(path), str(src), str(start)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        got = parse_formats(r.stdout)
        assert sorted(got) == sorted(FORMATS)
        levels, preds = G.bfs(n, Ap, Aj, src), G.bfs(n, Ap, Aj, src, mark_levels=False)
        vertex, last_levels, searches = G.pseudo_peripheral(n, Ap, Aj, start)
        p, _ = G.symmetric_rcm(n, Ap, Aj, start)
        count, components = G.connected_components(n, Ap, Aj)
        ni, nj, nx = G.symmetric_permute(M.csr_rows(Ap), Aj, np.arange(1, len(Aj) + 1, dtype=np.float64), p)
        for fmt in FORMATS:
            g = got[fmt]
            assert g["search"] == levels[1:] == preds[1:], (fmt, src)
            assert np.array_equal(g["levels"], levels[0]) and np.array_equal(g["preds"], preds[0]), (fmt, src)
            assert g["peripheral"] == (vertex, searches, vertex), (fmt, start)
            assert np.array_equal(g["last_levels"], last_levels) and np.array_equal(g["permutation"], p), (fmt, start)
            assert g["count"] == (count,) and np.array_equal(g["components"], components), fmt
            if fmt != "dia" or len(g["rows"]) or len(Aj) == 0:   # (DIA refuses a matrix of too many diagonals, as it does in the reference)
                assert np.array_equal(g["rows"], ni) and np.array_equal(g["cols"], nj) and np.array_equal(g["values"], nx), fmt


def test_graph_headers_compile_in_both_spaces(tmp_path):
    src = tmp_path / "good.cpp"
    src.write_text("#include <cusp/csr_matrix.h>\n#include <cusp/coo_matrix.h>\n#include <cusp/multiply.h>\n#include <cusp/graph/breadth_first_search.h>\n"
                   "#include <cusp/graph/pseudo_peripheral.h>\n#include <cusp/graph/symmetric_rcm.h>\n#include <cusp/graph/connected_components.h>\n"
                   "#include <cusp/permutation_matrix.h>\n"
                   "template <typename S> void f() { cusp::coo_matrix<int, float, S> G; cusp::csr_matrix<int, double, S> C; cusp::array1d<int, S> l; cusp::array1d<float, cusp::host_memory> h;\n"
                   "  cusp::graph::breadth_first_search(G, 0, l); cusp::graph::breadth_first_search(cusp::hip::par, C, 0, h, false);\n"
                   "  int v = cusp::graph::pseudo_peripheral_vertex(G); v += cusp::graph::pseudo_peripheral_vertex(C, l); v += cusp::graph::pseudo_peripheral_vertex(cusp::hip::par, G, h);\n"
                   "  v += cusp::graph::pseudo_peripheral_vertex(cusp::hip::par, C); (void)v;\n"
                   "  cusp::permutation_matrix<int, S> P, I(4), Q(4, l); cusp::permutation_matrix<int, cusp::host_memory> H(P); P.resize(7);\n"
                   "  cusp::graph::symmetric_rcm(G, P); cusp::graph::symmetric_rcm(cusp::hip::par, C, P); P.symmetric_permute(G); P.symmetric_permute(C);\n"
                   "  size_t c = cusp::graph::connected_components(G, l) + cusp::graph::connected_components(cusp::hip::par, C, h); (void)c;\n"
                   "  cusp::array1d<double, S> x, y; cusp::array1d<float, S> xf, yf; cusp::array1d<int, S> xi, yi;\n"
                   "  cusp::multiply(P, x, y); cusp::multiply(x, P, y); cusp::multiply(P, xf, yf); cusp::multiply(xi, P, yi); cusp::multiply(C, x, y); }\n"
                   "int main() { f<cusp::host_memory>(); f<cusp::device_memory>(); return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{INC}", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
