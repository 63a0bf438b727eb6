"""csr_wavev's equal-length tiles on an MI355X: a tile whose rows all have the longest row's length takes its row bounds from the
partition entry (no row offset is read); every other tile reads them as before.  Every case of tests/uniform_tiles_refs.py
(tests/test_uniform_tiles_refs.py shows what each contains) runs in f64 and f32 at V = 1, 2, 4, plain, accumulating onto a seeded y
and through the fused <y, w> entry of the CG loop; y must have the oracle host loop's bits
(reference arithmetic: cusp/system/detail/sequential/multiply/csr_spmv.h:42-74), the dot the fused-dot tolerance of
tests/test_round4_gpu.py against math.fsum."""
import math

import numpy as np
import pytest

import special_values as sv
import uniform_tiles_refs as ut

pytestmark = pytest.mark.gpu

_REF = {}


def reference(orc, name, tag):
    """Inputs and the host loop's results of a case, computed once and shared (read-only) by the V = 1, 2, 4 runs."""
    if (name, tag) not in _REF:
        dtype = np.float64 if tag == "f64" else np.float32
        Ap, Aj, cols, _ = ut.structure(name)
        Ax, x, y0, w = ut.vectors(name, dtype)
        want, want_acc = orc.spmv_csr(Ap, Aj, Ax, x), orc.spmv_csr(Ap, Aj, Ax, x, y0.copy())
        prod = (want.astype(np.float64) * w.astype(np.float64)).tolist()
        item = dict(Ap=Ap, Aj=Aj, cols=cols, Ax=Ax, x=x, y0=y0, w=w, want=want, want_acc=want_acc, dot=math.fsum(prod),
                    dot_abs=math.fsum(map(abs, prod)))
        for v in item.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[(name, tag)] = item
    return _REF[(name, tag)]


@pytest.mark.parametrize("V", ut.V_ALL)
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_uniform_tiles_bit_exact(cmi, orc, tag, V):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    tdt = torch.float64 if tag == "f64" else torch.float32
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the shared references stay read-only)
    ws = cmi.blas_workspace()
    for name in ut.CASES:
        R = reference(orc, name, tag)
        Ap, Aj = R["Ap"], R["Aj"]
        rows, cols, nnz = len(Ap) - 1, R["cols"], int(Ap[-1])
        max_len = int(np.diff(Ap.astype(np.int64)).max())
        if not ut.admits(max_len, V):
            continue
        what = f"{name} {tag} V={V} (uniform, other tiles: {ut.tile_counts(Ap, V)})"
        dAp, dAj, dAx, dx = dev(Ap), dev(Aj), dev(R["Ax"]), dev(R["x"])
        plan = cmi.Plan.csr(tdt, rows, cols, dAp, dAj, cfg=cmi.Config(kernel=cmi.CSR_STREAM_WAVEV, items_per_thread=V))
        c = plan.config()
        assert (c.kernel, c.items_per_thread) == (cmi.CSR_STREAM_WAVEV, V), (what, c)
        assert plan.info()["max_row_length"] == max_len, what
        y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y)
        sv.same_bits(y.cpu().numpy(), R["want"], what)
        y = dev(R["y0"])
        cmi.spmv_csr_plan(plan, dAp, dAj, dAx, dx, y, accumulate=True)
        sv.same_bits(y.cpu().numpy(), R["want_acc"], what + " accumulate")
        res = torch.zeros(1, dtype=torch.float64, device="cuda")
        y = torch.full((rows,), 9.0, dtype=tdt, device="cuda")
        cmi.spmv_csr_dot(rows, cols, dAp, dAj, dAx, dx, y, dev(R["w"]), res, ws, plan=plan)
        sv.same_bits(y.cpu().numpy(), R["want"], what + " fused dot: y")
        assert abs(res.item() - R["dot"]) <= 1e-9 * R["dot_abs"] + 1e-300, (what, res.item(), R["dot"])
