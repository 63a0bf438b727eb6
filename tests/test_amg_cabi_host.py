"""CPU tests (-m "not gpu") of the C-ABI of smoothed aggregation's set-up kernels (csrc/amg.hip): the exported symbols with
their prototypes and Python wrappers, and every refusal that must happen before a device call (host buffers only: on a
machine without a GPU anything that reached the device would come back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes

import pytest

INVALID = 1
CEILING = 2**31 - 1 - 65536
NAMES = ("csr_strength_symmetric", "csr_scale_rows", "aggregates_fit", "csr_elementwise", "relax_jacobi_presmooth")


def test_amg_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in NAMES:
        for suf in ("f64", "f32"):
            fn = getattr(L, f"cmi_{name}_{suf}")
            assert fn.argtypes is not None, f"cmi_{name}_{suf} has no prototype in binding.py"
        assert callable(getattr(cmi, name)), name


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_amg_argument_validation_without_a_device(cmi, suf):
    L = cmi.lib()
    strength, scale, fit, elementwise, presmooth = (getattr(L, f"cmi_{name}_{suf}") for name in NAMES)
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    p, q, r, s, t, u, v, w, x = (base + 4096 * i for i in range(9))
    ok_flag = ctypes.c_int(7)
    flag = ctypes.byref(ok_flag)

    def refused(fn, needle, *args):
        assert fn(*args) == INVALID, (fn.__name__, args)
        assert needle in L.cmi_last_error(), L.cmi_last_error()

    # (a) num_rows, num_cols, num_entries, Ap, Aj, Ax, theta, Sp, Sj, Sx, capacity, stream
    ok = (4, 4, 6, p, q, r, 0.25, s, t, u, 6, None)
    for pos in (0, 1, 2, 10):
        bad = list(ok)
        bad[pos] = -1
        refused(strength, b"negative", *bad)
    for pos, val in ((0, 2**31 - 1), (1, 2**31 - 1), (2, CEILING + 1)):
        bad = list(ok)
        bad[pos] = val
        bad[10] = max(val, 6)
        refused(strength, b"exceed", *bad)
    refused(strength, b"square", 4, 5, 6, p, q, r, 0.25, s, t, u, 6, None)
    refused(strength, b"capacity 5", 4, 4, 6, p, q, r, 0.25, s, t, u, 5, None)
    for pos in (3, 4, 5, 7, 8, 9):
        bad = list(ok)
        bad[pos] = None
        refused(strength, b"null", *bad)

    # (b) num_rows, num_entries, Ap, Ax, d, lambda, out, stream
    ok = (4, 6, p, q, r, 0.5, q, None)
    refused(scale, b"negative", -1, 6, p, q, r, 0.5, q, None)
    refused(scale, b"negative", 4, -1, p, q, r, 0.5, q, None)
    refused(scale, b"exceed", 2**31 - 1, 6, p, q, r, 0.5, q, None)
    refused(scale, b"exceed", 4, CEILING + 1, p, q, r, 0.5, q, None)
    refused(scale, b"without rows", 0, 6, p, q, r, 0.5, q, None)
    for pos in (2, 3, 4, 6):
        bad = list(ok)
        bad[pos] = None
        refused(scale, b"null", *bad)
    assert scale(4, 0, p, None, None, 0.5, None, None) == 0     # nothing to do: success without a device

    # (c) n, num_aggregates, aggregates, B, Tp, Tj, Tx, capacity, R, stream
    ok = (5, 2, p, q, r, s, t, 5, u, None)
    for pos in (0, 1, 7):
        bad = list(ok)
        bad[pos] = -1
        refused(fit, b"negative", *bad)
    refused(fit, b"exceed", CEILING + 1, 2, p, q, r, s, t, CEILING + 1, u, None)
    refused(fit, b"exceed", 5, 2**31 - 1, p, q, r, s, t, 5, u, None)
    refused(fit, b"capacity 4", 5, 2, p, q, r, s, t, 4, u, None)
    for pos in (2, 3, 4, 5, 6, 8):
        bad = list(ok)
        bad[pos] = None
        refused(fit, b"null", *bad)

    # (d) num_rows, num_cols, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, op, Cp, Cj, Cx, capacity, sorted_host, stream
    ok = (4, 5, 3, p, q, r, 2, s, t, u, 0, v, w, x, 5, flag, None)
    for pos in (0, 1, 2, 6, 14):
        bad = list(ok)
        bad[pos] = -1
        refused(elementwise, b"negative", *bad)
    for pos, val in ((0, 2**31 - 1), (1, 2**31 - 1), (2, CEILING + 1), (6, CEILING + 1), (6, CEILING - 2)):
        bad = list(ok)
        bad[pos] = val
        bad[14] = 2**31
        refused(elementwise, b"exceed", *bad)
    for op in (-1, 2):
        bad = list(ok)
        bad[10] = op
        refused(elementwise, b"op is", *bad)
    bad = list(ok)
    bad[14] = 4
    refused(elementwise, b"capacity 4", *bad)
    for pos in (3, 4, 5, 7, 8, 9, 11, 12, 13, 15):
        bad = list(ok)
        bad[pos] = None
        refused(elementwise, b"null", *bad)
    assert ok_flag.value == 7                                   # a refused call does not touch the flag

    # (e) n, d, b, omega, x, stream
    refused(presmooth, b"negative", -1, p, q, 0.5, r, None)
    refused(presmooth, b"exceed", 2**31, p, q, 0.5, r, None)
    for args in ((3, None, q, 0.5, r, None), (3, p, None, 0.5, r, None), (3, p, q, 0.5, None, None)):
        refused(presmooth, b"null", *args)
    assert presmooth(0, None, None, 0.5, None, None) == 0


def test_python_wrappers_refuse_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.csr_strength_symmetric(2, z, z[:2], v)              # host tensors: there is no CPU path
    with pytest.raises(TypeError):
        cmi.relax_jacobi_presmooth(v, v, 1.0, v)
