"""CPU tests (-m "not gpu") of the dense product's entry points (csrc/dense.hip): the two symbols and the Python callable exist, every refusal
is made with host buffers before any device call (a negative size, a leading dimension below the operand's rows, a null non-empty operand,
C overlapping A or B) and leaves a message, empty products are accepted without a device, cmi_version() is unchanged, and Python refuses
host tensors."""
import pytest

from test_multishift_cabi_host import Arena, refused


def test_dense_symbols_are_exported(cmi):
    L = cmi.lib()
    for suf in ("f64", "f32"):
        assert hasattr(L, f"cmi_dense_gemm_{suf}")
    assert callable(cmi.dense_gemm)
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_gemm_refuses_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    f = getattr(L, f"cmi_dense_gemm_{suf}")
    # (m, n, k, A, lda, B, ldb, C, ldc, stream): 8 x 3 <- (8 x 4) (4 x 3); A spans 40 elements at lda = 10, B 14 at ldb = 5, C 26 at ldc = 9
    A, B, C = a.take(3)
    good = [8, 3, 4, A, 10, B, 5, C, 9, None]
    for k in (0, 1, 2):
        bad = list(good)
        bad[k] = -1
        assert refused(L, f(*bad), b"negative"), k
    for k, ld in ((4, 7), (6, 3), (8, 7), (4, -1)):
        bad = list(good)
        bad[k] = ld
        assert refused(L, f(*bad), b"leading dimension"), (k, ld)
    for k in (3, 5, 7):
        bad = list(good)
        bad[k] = None
        assert refused(L, f(*bad), b"null"), k
    # C on A's first and last element, on B's last element, and A's / B's first element on C's last
    for k, other in ((7, A), (7, A + 37 * size), (7, B + 13 * size), (3, C + 25 * size), (5, C + 25 * size), (7, A - 25 * size)):
        bad = list(good)
        bad[k] = other
        assert refused(L, f(*bad), b"overlaps"), (k, other)
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(f(-1, *good[1:]))
    assert e.value.status == 1
    # nothing to write: accepted without a device, whatever the pointers
    assert f(0, 3, 4, None, 0, B, 5, None, 0, None) == 0
    assert f(8, 0, 4, A, 10, None, 4, None, 8, None) == 0
    assert f(0, 0, 0, None, 0, None, 0, None, 0, None) == 0
    # an empty operand needs neither an address nor a leading dimension, but C does
    assert refused(L, f(8, 3, 0, None, 0, None, 0, None, 9, None), b"null")
    assert refused(L, f(8, 3, 0, None, 0, None, 0, C, 7, None), b"leading dimension")


def test_dense_gemm_python_refuses_host_tensors(cmi):
    import torch
    for dt in (torch.float64, torch.float32):
        A, B, C = torch.zeros(12, dtype=dt), torch.zeros(6, dtype=dt), torch.zeros(8, dtype=dt)
        with pytest.raises(TypeError):
            cmi.dense_gemm(4, 2, 3, A, 4, B, 3, C, 4)
