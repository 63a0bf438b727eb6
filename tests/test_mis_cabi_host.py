"""CPU tests (-m "not gpu") of the C-ABI of the maximal independent set (csrc/mis.hip): the exported symbols with their
prototypes and Python wrappers, and every refusal that must happen before a device call (host buffers only: on a machine
without a GPU anything that reached the device would come back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes

import pytest

INVALID = 1
CEILING = 2**31 - 1 - 65536
NAMES = ("cmi_csr_ring_max_u64", "cmi_csr_maximal_independent_set", "cmi_csr_mis_aggregate")


def test_mis_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in NAMES:
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in binding.py"
    for name in ("csr_ring_max", "maximal_independent_set", "mis_aggregate"):
        assert callable(getattr(cmi, name)), name


def test_mis_argument_validation_without_a_device(cmi):
    L = cmi.lib()
    ring, mis, aggregate = (getattr(L, name) for name in NAMES)
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    p, q, r, s = (base + 4096 * i for i in range(4))
    size, rounds, count = ctypes.c_int64(7), ctypes.c_int(7), ctypes.c_int64(7)
    bs, br, bc = ctypes.byref(size), ctypes.byref(rounds), ctypes.byref(count)

    def refused(fn, needle, *args):
        assert fn(*args) == INVALID, (fn.__name__, args)
        assert needle in L.cmi_last_error(), L.cmi_last_error()

    # num_rows, num_entries, Ap, Aj, x, z, stream
    ok = (4, 6, p, q, r, s, None)
    for pos in (0, 1):
        bad = list(ok)
        bad[pos] = -1
        refused(ring, b"negative", *bad)
    refused(ring, b"exceed", 2**31 - 1, 6, p, q, r, s, None)
    refused(ring, b"exceed", 4, CEILING + 1, p, q, r, s, None)
    for pos in (2, 3, 4, 5):
        bad = list(ok)
        bad[pos] = None
        refused(ring, b"null", *bad)
    refused(ring, b"must not be x", 4, 6, p, q, r, r, None)
    assert ring(0, 0, None, None, None, None, None) == 0          # nothing to do: success without a device

    # num_rows, num_entries, Ap, Aj, k, seed, stencil, set_size, rounds, stream
    ok = (4, 6, p, q, 1, 0, r, bs, br, None)
    for pos in (0, 1):
        bad = list(ok)
        bad[pos] = -1
        refused(mis, b"negative", *bad)
    refused(mis, b"exceed", 2**31 - 1, 6, p, q, 1, 0, r, bs, br, None)
    refused(mis, b"exceed", 4, CEILING + 1, p, q, 1, 0, r, bs, br, None)
    refused(mis, b"k is negative", 4, 6, p, q, -1, 0, r, bs, br, None)
    for pos in (2, 3, 6, 7, 8):
        bad = list(ok)
        bad[pos] = None
        refused(mis, b"null", *bad)
    assert size.value == 7 and rounds.value == 7                # a refused call does not touch the host words
    assert mis(0, 0, None, None, 2, 0, None, bs, br, None) == 0 and size.value == 0 and rounds.value == 0

    # num_rows, num_entries, Ap, Aj, seed, aggregates, mis, num_aggregates, stream
    ok = (4, 6, p, q, 0, r, s, bc, None)
    for pos in (0, 1):
        bad = list(ok)
        bad[pos] = -1
        refused(aggregate, b"negative", *bad)
    refused(aggregate, b"exceed", 2**31 - 1, 6, p, q, 0, r, s, bc, None)
    refused(aggregate, b"exceed", 4, CEILING + 1, p, q, 0, r, s, bc, None)
    for pos in (2, 3, 5, 6, 7):
        bad = list(ok)
        bad[pos] = None
        refused(aggregate, b"null", *bad)
    assert count.value == 7
    assert aggregate(0, 0, None, None, 0, None, None, bc, None) == 0 and count.value == 0


def test_python_wrappers_refuse_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        cmi.maximal_independent_set((2, z, z[:2]))               # host tensors: there is no CPU path
    with pytest.raises(TypeError):
        cmi.mis_aggregate((2, z, z[:2]))
    with pytest.raises(TypeError):
        cmi.csr_ring_max(2, z, z[:2], torch.zeros(2, dtype=torch.int64))
