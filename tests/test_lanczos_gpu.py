"""GPU tests (-m gpu) of cusp::eigen::lanczos and cusp::blas::gemm on device_memory (tests/lanczos/test_lanczos_device.cpp): the host program's
unit tests (the identity / restart case and the growth case among them), the 16 x 12 and 33 x 31 solver cases fused and with
$CMI_LANCZOS_FUSED=0 under the bars (i)-(v) of tests/test_lanczos_host.py, the five formats and a linear_operator once, and gemm on
device_memory against the bits of the host_memory call.  Every program run is started under its own time limit.
Observed on an MI355X, fused and plain alike: value errors <= 1.6e-11 in double (33 x 31, LA 4) and <= 3.6e-7 in float (16 x 12);
max |E^T E - I| <= 0.16 m eps in double, 0.017 m eps in float; the restatement's step counts on every case."""
import subprocess

import pytest

import lanczos_refs as R
import special_values as sv
import test_lanczos_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_program(cmi, tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("lanczos_device"), "test_lanczos_device.cpp", "test_lanczos_device")


def test_lanczos_cpp_device_layer(device_program):
    r = subprocess.run([str(device_program)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert H.HOST_TESTS in r.stdout


def test_device_solver_cases_fused_and_plain(device_program):
    """Every 16 x 12 and 33 x 31 case on device_memory: the fused path and the $CMI_LANCZOS_FUSED=0 path each meet the host's bars."""
    r = subprocess.run([str(device_program), "cases"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = H.parse_cases(r.stdout)
    expected = H.expected_rows(device=True)
    assert len(rows) == 2 * len(expected)
    for k, (case, fmt) in enumerate(expected):
        fused, plain = rows[2 * k:2 * k + 2]
        assert (fused["case"], fused["format"], fused["run"]) == (case, fmt, "fused") and (plain["case"], plain["format"], plain["run"]) == (case, fmt, "plain")
        for row in (fused, plain):
            H.check_row(row)


def test_device_gemm_gives_the_bits_of_the_host_call(device_program, tmp_path):
    """cusp::blas::gemm on device_memory views (tight and padded pitches, k = 0, special values): the bits of gemm_ref, which the host_memory
    call is held to by tests/test_lanczos_host.py -- and of a host program built here, run on the same decks."""
    decks = H.gemm_decks()
    path = tmp_path / "gemm.txt"
    H.write_gemm_decks(path, decks)
    r = subprocess.run([str(device_program), "gemm", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    host = H.build(tmp_path, "test_lanczos_host.cpp", "test_lanczos_host")
    h = subprocess.run([str(host), "gemm", str(path)], capture_output=True, text=True, timeout=300)
    assert h.returncode == 0, (h.returncode, h.stderr[-2000:])
    got, on_host = H.parse_hex_lines(r.stdout), H.parse_hex_lines(h.stdout)
    assert len(got) == len(on_host) == len(decks)
    for g, w, deck in zip(got, on_host, decks):
        sv.same_bits(g.astype(deck[0]), w.astype(deck[0]), f"device against host {deck[1:7]}")
        sv.same_bits(g.astype(deck[0]), H.gemm_expected(deck), f"device against gemm_ref {deck[1:7]}")
