"""GPU test (-m gpu) of the routes the Krylov solvers of the header layer take on device_memory: tests/krylov_routes/routes.cpp runs every
(value type, operator form, solver) combination for exactly 30 iterations on poisson5pt(33, 31) and prints, per case, the iteration count,
the bits of the last residual norm and a hash of the solution.  The lines are compared with tests/golden/krylov_routes.json bit for bit.
That file was recorded with the headers and the library of the commit it names (twice, identical); the kernels and their launch order are
fixed, so a line that differs is a changed route or a changed argument in the header layer.

Operator forms: csr_matrix through its plan, csr_matrix with a forced configuration (no plan), coo, ell, dia, hyb whose COO part is empty,
hyb with a COO part, and a linear operator without a format tag.  Solvers: cg, cg with precond::diagonal, cr, bicgstab, cg_m; on CSR also
bicgstab_m, gmres(5) and each fused solver with its CMI_*_FUSED=0 switch.  cusp::array2d is no form: it has no device multiply."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "krylov_routes")
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "krylov_routes.json")


def test_every_krylov_route_gives_the_recorded_bits(cmi):
    exe = os.path.join(SRC, "bin", "routes")
    if not os.path.exists(exe):
        r = subprocess.run(["make", "-C", SRC], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "done"
    got = dict(line.split(" ", 1) for line in lines[:-1])
    with open(GOLDEN_FILE) as f:
        want = json.load(f)["cases"]
    assert len(want) == 92
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
