"""CPU tests (-m "not gpu") of the C-ABI of the graph algorithms (csrc/bfs.hip): the exported symbols with their prototypes and
Python wrappers, and every refusal that must happen before a device call (host buffers only: on a machine without a GPU
anything that reached the device would come back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes

import pytest

INVALID = 1
CEILING = 2**31 - 1 - 65536
SEARCHES = ("cmi_csr_breadth_first_search", "cmi_csr_pseudo_peripheral_vertex", "cmi_csr_symmetric_rcm")
COPIES = tuple(f"cmi_{kind}_{suffix}" for kind in ("gather", "scatter") for suffix in ("i32", "f32", "f64"))


def test_graph_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in SEARCHES + COPIES + ("cmi_bfs_levels_per_read",):
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in binding.py"
    for name in ("breadth_first_search", "pseudo_peripheral_vertex", "symmetric_rcm", "gather", "scatter", "bfs_levels_per_read"):
        assert callable(getattr(cmi, name)), name
    assert 1 <= cmi.bfs_levels_per_read() <= 1024 and cmi.bfs_levels_per_read() == L.cmi_bfs_levels_per_read()


def test_graph_argument_validation_without_a_device(cmi):
    L = cmi.lib()
    bfs, peripheral, rcm = (getattr(L, name) for name in SEARCHES)
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    p, q, r, s = (base + 4096 * i for i in range(4))
    reached, depth, vertex, searches = ctypes.c_int64(7), ctypes.c_int(7), ctypes.c_int64(7), ctypes.c_int(7)
    br, bd, bv, bs = (ctypes.byref(w) for w in (reached, depth, vertex, searches))

    def refused(fn, needle, *args):
        assert fn(*args) == INVALID, (fn.__name__, args)
        assert needle in L.cmi_last_error(), L.cmi_last_error()

    def common(fn, ok, pointers):
        """the refusals every search shares; ok[4] is the source / start vertex"""
        for pos in (0, 1):
            bad = list(ok)
            bad[pos] = -1
            refused(fn, b"negative", *bad)
        refused(fn, b"exceed", 2**31 - 1, *ok[1:])
        refused(fn, b"exceed", ok[0], CEILING + 1, *ok[2:])
        for pos in pointers:
            bad = list(ok)
            bad[pos] = None
            refused(fn, b"null", *bad)
        for src in (-1, ok[0], 2**40):
            bad = list(ok)
            bad[4] = src
            refused(fn, b"outside [0, num_rows)", *bad)
        refused(fn, b"", 0, 0, ok[2], None, 0, *ok[5:])            # no vertex at all: no source is inside

    # num_rows, num_entries, Ap, Aj, src, mark_levels, labels, reached, depth, stream
    for mark in (1, 0):
        common(bfs, (4, 6, p, q, 0, mark, r, br, bd, None), (2, 3, 6, 7, 8))
    # num_rows, num_entries, Ap, Aj, start, levels, vertex, searches, stream
    common(peripheral, (4, 6, p, q, 0, r, bv, bs, None), (2, 3, 5, 6, 7))
    # num_rows, num_entries, Ap, Aj, start, permutation, vertex, stream
    common(rcm, (4, 6, p, q, 0, r, bv, None), (2, 3, 5, 6))
    assert (reached.value, depth.value, vertex.value, searches.value) == (7, 7, 7, 7)   # a refused call does not touch the host words

    # n, m, map, in, out, stream
    for name in COPIES:
        fn = getattr(L, name)
        ok = (4, 6, p, q, r, None)
        for pos in (0, 1):
            bad = list(ok)
            bad[pos] = -1
            refused(fn, b"negative", *bad)
        refused(fn, b"exceed", 2**31 - 1, 6, p, q, r, None)
        refused(fn, b"exceed", 4, 2**31 - 1, p, q, r, None)
        for pos in (2, 3, 4):
            bad = list(ok)
            bad[pos] = None
            refused(fn, b"null", *bad)
        refused(fn, b"must not be in", 4, 6, p, q, q, None)
        assert fn(0, 0, None, None, None, None) == 0            # nothing to do: success without a device
        assert fn(0, 6, None, None, None, None) == 0


def test_python_wrappers_refuse_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    for fn in (cmi.breadth_first_search, cmi.pseudo_peripheral_vertex, cmi.symmetric_rcm):
        with pytest.raises(TypeError):
            fn(2, z, z[:2], 0)                                  # host tensors: there is no CPU path
    for fn in (cmi.gather, cmi.scatter):
        with pytest.raises(TypeError):
            fn(z, torch.zeros(3), 3)
