"""CPU tests (-m "not gpu") of the C-ABI of the semiring multiply (csrc/spmv_semiring.hip): the eight exported symbols with their prototypes
and Python wrappers, and every refusal that must happen before a device call (host buffers only: on a machine without a GPU anything that
reached the device would come back as a HIP error, not as CMI_ERROR_INVALID_VALUE)."""
import ctypes

import pytest

import semiring_refs as R

INVALID = 1
CEILING = 2**31 - 1 - 65536
FORMATS = ("csr", "ell", "dia", "coo")
NAMES = tuple(f"cmi_spmv_{fmt}_semiring_{suf}" for fmt in FORMATS for suf in ("f64", "f32"))
PLUS, MULTIPLIES, MINIMUM, MAXIMUM, PROJECT1ST, PROJECT2ND = range(6)


def test_the_eight_symbols_are_exported(cmi):
    L = cmi.lib()
    assert len(NAMES) == 8
    for name in NAMES:
        assert getattr(L, name).argtypes is not None, f"{name} has no prototype in binding.py"
    for fmt in FORMATS:
        assert callable(getattr(cmi, f"spmv_{fmt}_semiring")), fmt
    assert callable(cmi.spmv_semiring)
    assert [cmi.semiring_op(n) for n in R.COMBINES] == [R.OP_CODE[n] for n in R.COMBINES] == list(range(6))
    with pytest.raises(ValueError):
        cmi.semiring_op("times")


@pytest.mark.parametrize("suf", ("f64", "f32"))
def test_refusals_without_a_device(cmi, suf):
    L = cmi.lib()
    elem = 8 if suf == "f64" else 4
    buf = (ctypes.c_char * (1 << 16))()
    base = ctypes.addressof(buf)
    a, b, c, x, y0, y = (base + 8192 * i for i in range(6))

    def refused(fn, needle, *args):
        assert fn(*args) == INVALID, (needle, args)
        assert needle in L.cmi_last_error(), L.cmi_last_error()

    # the operands of each entry point with good values: (sizes..., three matrix arrays, x, y0, init, combine, reduce, y, stream)
    good = {"csr": [4, 4, 6, a, b, c, x, y0, 0.0, MULTIPLIES, PLUS, y, None],       # rows, cols, entries, Ap, Aj, Ax
            "coo": [4, 4, 6, a, b, c, x, y0, 0.0, MULTIPLIES, PLUS, y, None],       # rows, cols, entries, Ai, Aj, Ax
            "ell": [4, 4, 2, 4, b, c, x, y0, 0.0, MULTIPLIES, PLUS, y, None],       # rows, cols, width, pitch, Aj, Ax
            "dia": [4, 4, 3, 4, b, c, x, y0, 0.0, MULTIPLIES, PLUS, y, None]}       # rows, cols, diagonals, pitch, offsets, values
    sizes = {"csr": (0, 1, 2), "coo": (0, 1, 2), "ell": (0, 1, 2), "dia": (0, 1, 2)}
    COMB, RED, X, Y = 9, 10, 6, 11
    for fmt in FORMATS:
        fn = getattr(L, f"cmi_spmv_{fmt}_semiring_{suf}")

        def call_with(**changes):
            args = list(good[fmt])
            for pos, v in changes.items():
                args[int(pos[1:])] = v
            return args

        # an operation outside the enum, a projection as reduce
        for op in (-1, 6, 99):
            refused(fn, b"combine", *call_with(**{f"p{COMB}": op}))
        for op in (-1, PROJECT1ST, PROJECT2ND, 6):
            refused(fn, b"reduce", *call_with(**{f"p{RED}": op}))
        # negative sizes, sizes beyond the int32 ceiling of cmi_spmv_csr_*
        for pos in sizes[fmt]:
            refused(fn, b"negative", *call_with(**{f"p{pos}": -1}))
        refused(fn, b"exceed", *call_with(p0=2**31))
        refused(fn, b"exceed", *call_with(p1=2**31))
        refused(fn, b"exceed", *call_with(p2=CEILING + 1))
        if fmt in ("ell", "dia"):
            refused(fn, b"pitch", *call_with(p3=3))
        # y overlapping x (in part, too); y0 == y and y0 == x are allowed and reach the device, so they are not called here
        refused(fn, b"overlaps", *call_with(**{f"p{X}": y}))
        refused(fn, b"overlaps", *call_with(**{f"p{X}": y + elem * 3}))
        refused(fn, b"overlaps", *call_with(**{f"p{X}": y - elem * 3}))
        # a NULL array that the chosen operations read
        refused(fn, b"null", *call_with(**{f"p{Y}": None}))
        first = 3 if fmt in ("csr", "coo") else 4
        reads = {MULTIPLIES: (first, first + 1, first + 2, X) if fmt in ("csr", "coo") else (first, first + 1, X)}
        if fmt in ("csr", "coo"):      # index array, columns, values, x
            reads[PROJECT2ND] = (first, first + 1, X)
            reads[PROJECT1ST] = (first, first + 2)
        else:                          # columns / offsets, values, x
            reads[PROJECT2ND] = (first, X)
            reads[PROJECT1ST] = (first, first + 1)
        for combine, positions in reads.items():
            for pos in positions:
                refused(fn, b"null", *call_with(**{f"p{COMB}": combine, f"p{pos}": None}))
        # num_rows == 0: success, nothing launched, whatever else is given
        args = call_with(p0=0)
        assert fn(*args) == 0
        assert fn(0, 0, 0, 0 if fmt in ("ell", "dia") else None, None, None, None, None, 0.0, PROJECT2ND, MAXIMUM, None, None) == 0


def test_python_wrappers_refuse_bad_operands(cmi):
    import torch
    z = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(TypeError):
        cmi.spmv_csr_semiring(2, 3, z, z, v, v, v[:2], "plus", "minimum")       # host tensors: there is no CPU path
    with pytest.raises(TypeError):
        cmi.spmv_semiring(object(), v, v)
