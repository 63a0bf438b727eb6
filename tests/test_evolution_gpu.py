"""Evolution strength of connection (csrc/evolution.hip) on the MI355X, through the C-ABI, against tests/evolution_refs.py:
the transpose map, the masked product and the three arrays of S, structure exactly and values bit for bit
(special_values.same_bits), f64 and f32.  No tolerance anywhere.

The masked product stages rows in LDS: rows of up to 64 entries in one piece (the span of a wave's 64 entries), a longer row in
chunks of CHUNK = 192 entries.  `arrow 70` has one row longer than a wave and shorter than a chunk, `arrow 200` one row of two chunks.
"""
import ctypes

import numpy as np
import pytest

import evolution_refs as E
from special_values import same_bits

pytestmark = pytest.mark.gpu
DT = [np.float64, np.float32]
CHUNK = 192
NAMES = list(E.decks(np.float64))


def dev(a, torch):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def check_csr(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: row offsets differ"
    assert got[0][-1] == len(got[1]) == len(got[2]), what
    assert np.array_equal(got[1], want[1]), f"{what}: column indices differ"
    same_bits(got[2], want[2], what)


def free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def assert_memory_returns(cmi, torch, call):
    """`call` leaves the device bytes held by the library where they were (the idiom of tests/test_amg_gpu.py)."""
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


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def restated():
    """Every deck with its restatement, computed once and left unchanged."""
    return {dt: {name: (d, E.evolution_strength(*d)) for name, d in E.decks(dt).items()} for dt in DT}


def test_the_decks_cross_the_kernel_paths():
    d = E.decks(np.float64)
    assert np.diff(d["arrow 70"][1]).max() == 70 > 64 and np.diff(d["arrow 200"][1]).max() == 200 > CHUNK
    assert d["diagonal 65"][0] == 65 and len(d["tridiagonal 130 with gaps"][2]) == 3 * 130 - 2 - 3 and d["empty"][0] == 0


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", NAMES)
def test_deck_equals_the_restatement_bit_for_bit(cmi, torch_cuda, restated, dtype, name):
    torch = torch_cuda
    (n, Ap, Aj, Ax, B, rho, eps), want = restated[dtype][name]
    dAp, dAj = dev(Ap, torch), dev(Aj, torch)
    tpos = cmi.csr_transpose_positions(n, dAp, dAj)
    assert tpos is not None, "reported as non-conforming"
    assert np.array_equal(tpos.cpu().numpy(), want["tpos"]), "tpos differs"
    v = want["v"]
    data = cmi.csr_masked_product(n, dAp, dAj, dev(v, torch), dev(v[want["tpos"]], torch))
    same_bits(data.cpu().numpy(), want["data"], "masked product")
    got = cmi.csr_evolution_strength(n, dAp, dAj, dev(Ax, torch), dev(B, torch), rho, eps)
    assert got is not None, "reported as non-conforming"
    check_csr(host(got), want["S"], name)


@pytest.mark.parametrize("dtype", DT)
def test_masked_product_with_general_operands(cmi, torch_cuda, dtype):
    """Vx and Wx unrelated to each other, rows from empty to several chunks, more than one wave of entries, a column outside the matrix."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    n = 300
    lens = np.r_[rng.integers(0, 9, size=140), [63, 64, 65, 0, 193, 0, 0, 64, 300, 129], rng.integers(0, 9, size=150)]
    rows = [np.sort(rng.choice(n, size=l, replace=False)) for l in lens]
    Ap = np.r_[0, np.cumsum(lens)].astype(np.int32)
    Aj = np.concatenate(rows).astype(np.int32)
    Vx, Wx = rng.standard_normal(len(Aj)).astype(dtype), rng.standard_normal(len(Aj)).astype(dtype)
    want = E.masked_product(n, Ap, Aj, Vx, Wx)
    got = cmi.csr_masked_product(n, dev(Ap, torch), dev(Aj, torch), dev(Vx, torch), dev(Wx, torch))
    same_bits(got.cpu().numpy(), want, "general operands")
    assert np.count_nonzero(want) > len(Aj) // 4
    Aj2 = Aj.copy()
    Aj2[Ap[5]:Ap[6]][-1:] = n + 3                                            # the last entry of row 5 points outside: its product is 0
    same_bits(cmi.csr_masked_product(n, dev(Ap, torch), dev(Aj2, torch), dev(Vx, torch), dev(Wx, torch)).cpu().numpy(), E.masked_product(n, Ap, Aj2, Vx, Wx), "column outside")


def test_nonconforming_patterns_come_back_flagged_and_write_nothing(cmi, torch_cuda):
    torch = torch_cuda
    L = cmi.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for what, (n, Ap, Aj) in E.nonconforming().items():
        dAp, dAj = dev(Ap, torch), dev(Aj, torch)
        assert cmi.csr_transpose_positions(n, dAp, dAj) is None, what
        Ax, B = dev(np.ones(len(Aj)), torch), dev(np.ones(n), torch)
        assert cmi.csr_evolution_strength(n, dAp, dAj, Ax, B, 1.5) is None, what
        Sp = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        Sj = torch.full((len(Aj),), -7, dtype=torch.int32, device="cuda")
        Sx = torch.full((len(Aj),), -7.0, dtype=torch.float64, device="cuda")
        ok = ctypes.c_int(5)
        cmi.check(L.cmi_csr_evolution_strength_f64(n, len(Aj), vp(dAp), vp(dAj), vp(Ax), vp(B), 1.5, 4.0, vp(Sp), vp(Sj), vp(Sx), len(Aj), ctypes.byref(ok), None))
        torch.cuda.synchronize()
        assert ok.value == 0 and (Sp == -7).all() and (Sj == -7).all() and (Sx == -7).all(), what


def test_device_memory_returns_after_every_call(cmi, torch_cuda):
    torch = torch_cuda
    N, Ap, Aj, Ax = E.diffusion(60, 60, 1e-3, 0.0, "FE", np.float64)
    d = [dev(a, torch) for a in (Ap, Aj, Ax)]
    B = dev(np.ones(N), torch)
    unsorted = dev(Aj[::-1].copy(), torch)
    for call in (lambda: cmi.csr_transpose_positions(N, d[0], d[1]),
                 lambda: cmi.csr_masked_product(N, d[0], d[1], d[2], d[2]),
                 lambda: cmi.csr_evolution_strength(N, *d, B, 1.9),
                 lambda: cmi.csr_evolution_strength(N, *d, B, 1.9, float("inf")),
                 lambda: cmi.csr_evolution_strength(N, d[0], unsorted, d[2], B, 1.9)):
        assert_memory_returns(cmi, torch, call)


def test_evolution_device_layer_program(cmi, torch_cuda, tmp_path):
    """tests/evolution/test_evolution_device.cpp, once, in a child process under its own time limit: the measure on device_memory
    against host_memory of the same program bit for bit (rho supplied), the 7 x 5 facts with rho estimated on the device, the
    refusals, diffusion into the five formats, and smoothed aggregation with evolution strength as cg's preconditioner."""
    import os
    import subprocess
    from conftest import ROOT
    inc, libd = os.path.join(ROOT, "cusp-autotuned_amd", "include"), os.path.join(ROOT, "cusp-autotuned_amd", "lib")
    exe = tmp_path / "test_evolution_device"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off",
                        f"-I{inc}", f"-I{os.path.join(ROOT, 'tests', 'cpp')}", os.path.join(ROOT, "tests", "evolution", "test_evolution_device.cpp"),
                        "-o", str(exe), f"-L{libd}", "-lcusp_mi355x", f"-Wl,-rpath,{libd}", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "16 tests, 0 failed" in r.stdout
