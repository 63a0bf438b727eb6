"""CPU tests (-m "not gpu") of the LOBPCG entry points of csrc/lobpcg.hip: the six symbols and their Python callables exist, every refusal is
made with host buffers before any device call (a negative n, a null required array, an output range that overlaps another output or an
input) and leaves a message, cmi_version() is unchanged, and Python refuses host tensors."""
import ctypes

import pytest

from test_multishift_cabi_host import Arena, refused

ENTRIES = ("cmi_lobpcg_residual", "cmi_lobpcg_gram", "cmi_lobpcg_update")
CALLABLES = ("lobpcg_residual", "lobpcg_gram", "lobpcg_update")


def test_lobpcg_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in ENTRIES:
        for suf in ("f64", "f32"):
            assert hasattr(L, f"{name}_{suf}")
    for fn in CALLABLES:
        assert callable(getattr(cmi, fn))
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_residual_refuses_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    f = getattr(L, f"cmi_lobpcg_residual_{suf}")
    # (n, lambda_dev, x, ax, r, rr_dev, rr_host_mirror, workspace, stream)
    lam, x, ax, r, rr, ws = a.take(6)
    good = [32, lam, x, ax, r, rr, None, ws, None]
    assert refused(L, f(-1, *good[1:]), b"negative")
    for k in (1, 2, 3, 4, 5, 7):
        bad = list(good)
        bad[k] = None
        assert refused(L, f(*bad), b"null"), k
    for k, other in ((4, x), (4, ax + 31 * size), (4, ax - 31 * size), (5, lam), (5, x + 8), (4, rr)):   # r on x, on ax's last / first element, rr on lambda, on x, r on rr
        bad = list(good)
        bad[k] = other
        assert refused(L, f(*bad), b"overlaps"), (k, other)
    assert refused(L, f(0, None, None, None, None, rr, None, ws, None), b"null")   # n == 0 still needs its scalars
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(f(-1, *good[1:]))
    assert e.value.status == 1


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_gram_refuses_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    f = getattr(L, f"cmi_lobpcg_gram_{suf}")
    # (n, pp_dev, x, w, aw, p, ap, gram_dev, workspace, stream)
    pp, x, w, aw, p, ap, gram, ws = a.take(8)
    good = [32, pp, x, w, aw, p, ap, gram, ws, None]
    assert refused(L, f(-1, *good[1:]), b"negative")
    for k in (1, 2, 3, 4, 5, 6, 7, 8):
        bad = list(good)
        bad[k] = None
        assert refused(L, f(*bad), b"null"), k
    first = [32, None, x, w, aw, None, None, gram, ws, None]     # the first iteration's form: only x, w, aw are needed
    for k in (2, 3, 4, 7, 8):
        bad = list(first)
        bad[k] = None
        assert refused(L, f(*bad), b"null"), k
    for k, other in ((5, ap), (5, x), (6, aw + 31 * size), (6, w - 31 * size), (7, pp), (7, pp - 7 * 8), (7, x + 8), (5, gram + 7 * 8)):
        bad = list(good)
        bad[k] = other
        assert refused(L, f(*bad), b"overlaps"), (k, other)
    # three sums without p: gram_dev may sit 3 doubles in front of an input, not 2
    assert refused(L, f(32, None, x, w, aw, None, None, x - 2 * 8, ws, None), b"overlaps")


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_update_refuses_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    f = getattr(L, f"cmi_lobpcg_update_{suf}")
    # (n, cx, cr, cp, first, lambda_new, w, aw, p, ap, x, ax, r, scalars_dev, rr_host_mirror, workspace, stream)
    w, aw, p, ap, x, ax, r, sc, ws = a.take(9)
    head = [32, 0.5, -2.0, 0.25, 0, 3.0]
    good = head + [w, aw, p, ap, x, ax, r, sc, None, ws, None]
    assert refused(L, f(-1, *good[1:]), b"negative")
    for k in (6, 7, 8, 9, 10, 11, 13, 15):
        bad = list(good)
        bad[k] = None
        assert refused(L, f(*bad), b"null"), k
    for k, other in ((8, ap), (9, x), (10, ax + 31 * size), (11, r - 31 * size), (12, w), (12, aw + 31 * size), (8, w), (13, p + 8), (13, aw - 8), (12, sc + 8)):
        bad = list(good)
        bad[k] = other
        assert refused(L, f(*bad), b"overlaps"), (k, other)
    # r == NULL is a form of the call, not an error: nothing but the missing device stands between it and the launch
    no_r = list(good)
    no_r[12] = None
    no_r[8] = no_r[9]
    assert refused(L, f(*no_r), b"overlaps")


def test_lobpcg_python_refuses_host_tensors(cmi):
    import torch
    for dt in (torch.float64, torch.float32):
        v = [torch.zeros(8, dtype=dt) for _ in range(7)]
        d = [torch.zeros(8, dtype=torch.float64) for _ in range(3)]
        with pytest.raises(TypeError):
            cmi.lobpcg_residual(d[0][:1], v[0], v[1], v[2], d[1][:1], d[2])
        with pytest.raises(TypeError):
            cmi.lobpcg_gram(d[0][:1], v[0], v[1], v[2], v[3], v[4], d[1], d[2])
        with pytest.raises(TypeError):
            cmi.lobpcg_update(0.5, -2.0, 0.25, False, 3.0, *v, d[1][:2], d[2])
