"""CPU tests (-m "not gpu") of the multi-shift entry points of csrc/krylov_m.hip: the ten symbols and their Python callables exist,
every refusal is made with host buffers before any device call (a negative n or num_shifts, a null array, ld < n, an output range that
overlaps another output or an input), the no-op cases return 0, cmi_version() is unchanged, and Python refuses host tensors."""
import ctypes

import pytest

ENTRIES = ("cmi_cg_m_coefficients", "cmi_cg_m_update_xp", "cmi_bicgstab_m_s", "cmi_bicgstab_m_coefficients", "cmi_bicgstab_m_update_xs")
CALLABLES = ("cg_m_coefficients", "cg_m_update_xp", "bicgstab_m_s", "bicgstab_m_coefficients", "bicgstab_m_update_xs")


def test_multishift_symbols_are_exported(cmi):
    L = cmi.lib()
    for name in ENTRIES:
        for suf in ("f64", "f32"):
            assert hasattr(L, f"{name}_{suf}")
    for fn in CALLABLES:
        assert callable(getattr(cmi, fn))
    assert callable(cmi.krylov.cg_m)
    assert cmi.version() == 400   # unchanged: callers find the feature by symbol


class Arena:
    """Disjoint 4 KiB host ranges, 16-byte aligned; never dereferenced by a refused call."""

    def __init__(self):
        self.buf = (ctypes.c_char * (1 << 18))()
        self.base = ctypes.addressof(self.buf)
        self.base += -self.base % 16
        self.next = 0

    def take(self, count=1):
        out = [self.base + (self.next + i) * 4096 for i in range(count)]
        self.next += count
        return out if count > 1 else out[0]


def refused(L, status, word):
    return status == 1 and word in L.cmi_last_error()


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_cg_m_entries_refuse_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    coef = getattr(L, f"cmi_cg_m_coefficients_{suf}")
    # (num_shifts, rsq_old, pAp, rsq_new, state, sigma, zeta_m1, zeta_0, beta_s, alpha_s, stream)
    ro, pp, rn, st, sg, zm, z0, bs, al = a.take(9)
    assert refused(L, coef(-1, ro, pp, rn, st, sg, zm, z0, bs, al, None), b"negative")
    assert refused(L, coef(3, None, pp, rn, st, sg, zm, z0, bs, al, None), b"null")
    assert refused(L, coef(3, ro, pp, rn, None, sg, zm, z0, bs, al, None), b"null")
    assert refused(L, coef(0, ro, pp, None, st, None, None, None, None, None, None), b"null")
    for k in range(5, 10):
        args = [3, ro, pp, rn, st, sg, zm, z0, bs, al, None]
        args[k] = None
        assert refused(L, coef(*args), b"null"), k
    assert refused(L, coef(3, ro, pp, rn, st, sg, zm, zm, bs, al, None), b"overlaps")                 # two outputs
    assert refused(L, coef(3, ro, pp, rn, st, sg, zm, z0, bs, bs + 2 * size, None), b"overlaps")      # ... by one element
    assert refused(L, coef(3, ro, pp, rn, st, sg, zm, z0, sg, al, None), b"overlaps")                 # an output on an input
    assert refused(L, coef(3, ro, pp, rn, ro, sg, zm, z0, bs, al, None), b"overlaps")                 # state on a scalar
    assert refused(L, coef(3, ro, pp, rn, st, sg, st + size, z0, bs, al, None), b"overlaps")          # zeta_m1 on state[1]

    xp = getattr(L, f"cmi_cg_m_update_xp_{suf}")
    # (n, num_shifts, ld, state, beta_s, alpha_s, zeta_0, r, p0, x, p_s, stream)
    st, bs, al, z0, r, p0 = a.take(6)
    x, _, ps, _ = a.take(4)   # two pages each: 2 shifts x ld 40 x 8 bytes fit
    assert refused(L, xp(-1, 2, 40, st, bs, al, z0, r, p0, x, ps, None), b"negative")
    assert refused(L, xp(32, -2, 40, st, bs, al, z0, r, p0, x, ps, None), b"negative")
    assert refused(L, xp(32, 2, 31, st, bs, al, z0, r, p0, x, ps, None), b"ld < n")
    for k in (4, 5, 6, 7, 9, 10):
        args = [32, 2, 40, st, bs, al, z0, r, p0, x, ps, None]
        args[k] = None
        assert refused(L, xp(*args), b"null"), k
    assert refused(L, xp(32, 2, 40, None, bs, al, z0, r, p0, x, ps, None), b"state")                  # p0 needs state[1]
    assert refused(L, xp(32, 2, 40, st, bs, al, z0, r, p0, x, x, None), b"overlaps")
    assert refused(L, xp(32, 2, 40, st, bs, al, z0, r, p0, x, x + (40 + 31) * size, None), b"overlaps")   # the last element of shift 1
    assert refused(L, xp(32, 2, 40, st, bs, al, z0, r, r, x, ps, None), b"overlaps")                  # p0 on r
    assert refused(L, xp(32, 2, 40, st, bs, al, z0, x + 40 * size, p0, x, ps, None), b"overlaps")     # r inside x's second shift
    assert refused(L, xp(32, 2, 40, st, bs, al, ps, r, p0, x, ps, None), b"overlaps")                 # a coefficient array on p_s
    # nothing to do: no device call, status 0
    assert xp(0, 2, 0, None, None, None, None, None, None, None, None, None) == 0
    assert xp(0, 0, 0, None, None, None, None, None, None, None, None, None) == 0
    assert xp(32, 0, 0, None, None, None, None, None, None, None, None, None) == 0                     # no shift and no p0
    with pytest.raises(cmi.CmiError) as e:
        cmi.check(xp(-1, 2, 40, st, bs, al, z0, r, p0, x, ps, None))
    assert e.value.status == 1


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_bicgstab_m_entries_refuse_bad_arguments_without_a_device(cmi, suf):
    L = cmi.lib()
    a = Arena()
    size = 8 if suf == "f64" else 4
    s = getattr(L, f"cmi_bicgstab_m_s_{suf}")
    r1, As, s0 = a.take(3)
    assert refused(L, s(-1, 1.0, 1.0, r1, As, s0, None), b"negative")
    for k in (3, 4, 5):
        args = [8, 1.0, 1.0, r1, As, s0, None]
        args[k] = None
        assert refused(L, s(*args), b"null"), k
    assert refused(L, s(8, 1.0, 1.0, r1, As, r1 + 7 * size, None), b"overlaps")
    assert refused(L, s(8, 1.0, 1.0, r1, s0, s0, None), b"overlaps")
    assert s(0, 1.0, 1.0, None, None, None, None) == 0

    coef = getattr(L, f"cmi_bicgstab_m_coefficients_{suf}")
    # (num_shifts, beta_m1, beta_0, alpha_old, alpha_new, chi_0, sigma, zeta_m1, zeta_0, rho_0, zeta_1, beta_s, chi_s, rho_1, alpha_s, stream)
    arr = a.take(9)
    sc = [1.0, -1.0, 0.0, 0.5, 0.5]
    assert refused(L, coef(-1, *sc, *arr, None), b"negative")
    for k in range(9):
        bad = list(arr)
        bad[k] = None
        assert refused(L, coef(3, *sc, *bad, None), b"null"), k
    for i, j in ((4, 5), (4, 0), (8, 3), (6, 2)):   # output on output, outputs on inputs
        bad = list(arr)
        bad[i] = arr[j] + (2 * size if (i, j) == (8, 3) else 0)
        assert refused(L, coef(3, *sc, *bad, None), b"overlaps"), (i, j)
    assert coef(0, *sc, *([None] * 9), None) == 0

    xs = getattr(L, f"cmi_bicgstab_m_update_xs_{suf}")
    # (n, num_shifts, ld, beta_s, chi_s, rho_0, zeta_m1, zeta_0, alpha_s, rho_1, zeta_1, r_0, r_1, w_1, x, s_s, stream)
    small = a.take(11)
    x, _, ss, _ = a.take(4)
    good = [*small, x, ss]
    assert refused(L, xs(-1, 2, 40, *good, None), b"negative")
    assert refused(L, xs(32, -1, 40, *good, None), b"negative")
    assert refused(L, xs(32, 2, 31, *good, None), b"ld < n")
    for k in range(13):
        bad = list(good)
        bad[k] = None
        assert refused(L, xs(32, 2, 40, *bad, None), b"null"), k
    for i, j, off in ((12, 11, 0), (12, 11, (40 + 31) * size), (11, 9, 0), (2, 6, 0), (3, 4, size), (8, 11, 40 * size)):
        bad = list(good)
        bad[i] = good[j] + off
        assert refused(L, xs(32, 2, 40, *bad, None), b"overlaps"), (i, j)
    assert xs(0, 2, 0, *([None] * 13), None) == 0
    assert xs(32, 0, 40, *([None] * 13), None) == 0


def test_multishift_python_refuses_host_tensors(cmi):
    import torch
    for dt in (torch.float64, torch.float32):
        v = [torch.zeros(8, dtype=dt) for _ in range(14)]
        d = [torch.zeros(1, dtype=torch.float64) for _ in range(3)]
        with pytest.raises(TypeError):
            cmi.cg_m_coefficients(d[0], d[1], d[2], v[0][:2], v[1][:2], v[2][:2], v[3][:2], v[4][:2], v[5][:2])
        with pytest.raises(TypeError):
            cmi.cg_m_update_xp(4, 4, v[0][:2], v[1][:2], v[2][:2], v[3][:2], v[4][:4], v[5][:4], v[6], v[7])
        with pytest.raises(TypeError):
            cmi.bicgstab_m_s(1.0, 1.0, v[0], v[1], v[2])
        with pytest.raises(TypeError):
            cmi.bicgstab_m_coefficients(1.0, -1.0, 0.0, 0.5, 0.5, *[t[:2] for t in v[:9]])
        with pytest.raises(TypeError):
            cmi.bicgstab_m_update_xs(4, 4, *[t[:2] for t in v[:8]], v[8][:4], v[9][:4], v[10][:4], v[11], v[12])
