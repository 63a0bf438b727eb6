"""CPU tests (-m "not gpu") of the C-ABI of evolution strength of connection (csrc/evolution.hip): the exported symbols with
their prototypes and Python wrappers, and every refusal that must happen before a device call (host buffers only: on a
machine without a GPU anything that reached the device would come back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes

import pytest

INVALID = 1
CEILING = 2**31 - 1 - 65536


def test_evolution_symbols_are_exported(cmi):
    L = cmi.lib()
    assert L.cmi_csr_transpose_positions.argtypes is not None
    for name in ("csr_masked_product", "csr_evolution_strength"):
        for suf in ("f64", "f32"):
            assert getattr(L, f"cmi_{name}_{suf}").argtypes is not None, f"cmi_{name}_{suf} has no prototype in binding.py"
    for name in ("csr_transpose_positions", "csr_masked_product", "csr_evolution_strength"):
        assert callable(getattr(cmi, name)), name


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_evolution_argument_validation_without_a_device(cmi, suf):
    L = cmi.lib()
    tpos, product, measure = L.cmi_csr_transpose_positions, getattr(L, f"cmi_csr_masked_product_{suf}"), getattr(L, f"cmi_csr_evolution_strength_{suf}")
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    p, q, r, s, t, u, v = (base + 4096 * i for i in range(7))
    ok_flag = ctypes.c_int(7)
    flag = ctypes.byref(ok_flag)

    def refused(fn, needle, *args):
        assert fn(*args) == INVALID, (fn.__name__, args)
        assert needle in L.cmi_last_error(), L.cmi_last_error()

    # num_rows, Ap, Aj, tpos, conforming_host, stream
    refused(tpos, b"negative", -1, p, q, r, flag, None)
    refused(tpos, b"exceed", 2**31 - 1, p, q, r, flag, None)
    refused(tpos, b"null", 4, None, q, r, flag, None)
    refused(tpos, b"null", 4, p, q, r, None, None)

    # num_rows, Ap, Aj, Vx, Wx, out, stream
    refused(product, b"negative", -1, p, q, r, s, t, None)
    refused(product, b"exceed", 2**31 - 1, p, q, r, s, t, None)
    refused(product, b"null", 4, None, q, r, s, t, None)

    # num_rows, num_entries, Ap, Aj, Ax, B, rho_DinvA, epsilon, Sp, Sj, Sx, capacity, conforming_host, stream
    ok = (4, 6, p, q, r, s, 1.5, 4.0, t, u, v, 6, flag, None)
    for pos in (0, 1, 11):
        bad = list(ok)
        bad[pos] = -1
        refused(measure, b"negative", *bad)
    for pos, val in ((0, 2**31 - 1), (1, CEILING + 1)):
        bad = list(ok)
        bad[pos] = val
        bad[11] = max(val, 6)
        refused(measure, b"exceed", *bad)
    refused(measure, b"without rows", 0, 6, p, q, r, s, 1.5, 4.0, t, u, v, 6, flag, None)
    bad = list(ok)
    bad[11] = 5
    refused(measure, b"capacity 5", *bad)
    for rho in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        bad = list(ok)
        bad[6] = rho
        refused(measure, b"rho_DinvA", *bad)
    for pos in (2, 3, 4, 5, 8, 9, 10, 12):
        bad = list(ok)
        bad[pos] = None
        refused(measure, b"null", *bad)
    assert ok_flag.value == 7                                   # a refused call does not touch the flag


def test_python_wrappers_refuse_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(2, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.csr_transpose_positions(2, z, z[:2])                # host tensors: there is no CPU path
    with pytest.raises(TypeError):
        cmi.csr_masked_product(2, z, z[:2], v, v)
    with pytest.raises(TypeError):
        cmi.csr_evolution_strength(2, z, z[:2], v, v, 1.5)
