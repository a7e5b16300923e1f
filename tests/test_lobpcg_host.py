"""CPU: the host side of pysparse.eigen.lobpcg -- the small generalised eigenproblem behind the Rayleigh-Ritz step
(Cholesky of the mass Gram matrix, reduction to standard form, cyclic Jacobi) through the test hook psp_debug_gen_ritz, and
the import / signature / argument validation of the Python surface and of the C entry point.  Nothing here needs a GPU.

Bound of the hook (m the order): 64 m eps ||GA||_2 ||GM^-1||_2 for the eigenvalues against scipy.linalg.eigh(GA, GM), and
the same for C' GM C - I and C' GA C - diag(lambda)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.linalg

EPS = np.finfo(np.float64).eps


def lib():
    from pysparse_amd import _capi
    return _capi.lib()


def gen_ritz(GA, GM, ld=None):
    m = GA.shape[0]
    ld = ld or m
    a, g = np.full((m, ld), np.nan), np.full((m, ld), np.nan)  # column-major: a[c, r] = GA[r, c]
    a[:, :m], g[:, :m] = GA.T, GM.T
    lam, Cb = np.full(m, np.nan), np.full((m, ld), np.nan)
    rc = lib().psp_debug_gen_ritz(m, a.ctypes.data, g.ctypes.data, ld, lam.ctypes.data, Cb.ctypes.data)
    return rc, lam, Cb[:, :m].T.copy(), Cb[:, m:]


@pytest.mark.parametrize("m", [1, 2, 7, 24, 96])
def test_gen_ritz_against_scipy(m):
    rng = np.random.default_rng(m)
    B = rng.standard_normal((m, m))
    GA = (B + B.T) / 2
    B = rng.standard_normal((m, m))
    GM = B.T @ B + np.eye(m)
    rc, lam, Cm, pad = gen_ritz(GA, GM, ld=m + 3)
    assert rc == 0, lib().psp_last_error()
    assert np.all(np.isnan(pad)), "wrote behind the m rows of a column"
    ref = scipy.linalg.eigh(GA, GM, eigvals_only=True)
    bound = 64 * m * EPS * np.linalg.norm(GA, 2) * np.linalg.norm(np.linalg.inv(GM), 2)
    err = np.abs(lam - ref).max()
    orth = np.abs(Cm.T @ GM @ Cm - np.eye(m)).max()
    diag = np.abs(Cm.T @ GA @ Cm - np.diag(lam)).max()
    print("m=%d: eigenvalues %.3e, C'GM C - I %.3e, C'GA C - diag %.3e, bound %.3e" % (m, err, orth, diag, bound))
    assert np.all(np.diff(lam) >= 0)
    assert err <= bound and orth <= bound and diag <= bound


def test_gen_ritz_refuses_an_indefinite_mass_matrix():
    GA = np.eye(3)
    for GM in (np.diag([1.0, -1.0, 1.0]), np.zeros((3, 3)), np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]])):
        rc = gen_ritz(GA, GM)[0]
        assert rc != 0 and b"positive definite" in lib().psp_last_error()
    a = np.zeros(4)
    assert lib().psp_debug_gen_ritz(0, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data) != 0
    assert lib().psp_debug_gen_ritz(129, a.ctypes.data, a.ctypes.data, 129, a.ctypes.data, a.ctypes.data) != 0
    assert lib().psp_debug_gen_ritz(2, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data) != 0


# ---------------------------------------------------------------------- the Python surface

def test_import_signature_and_alias():
    from pysparse.eigen import lobpcg
    import pysparse.eigen.lobpcg as mod
    import pysparse_amd.eigen.lobpcg as amd
    assert mod is lobpcg and amd is lobpcg and callable(lobpcg.lobpcg)
    sig = inspect.signature(lobpcg.lobpcg)
    assert list(sig.parameters) == ["A", "M", "K", "k", "tol", "itmax", "X0"]
    assert sig.parameters["X0"].default is None
    assert all(p.default is inspect.Parameter.empty for name, p in sig.parameters.items() if name != "X0")


def test_jdsym_and_lobpcg_share_the_operand_helper():
    from pysparse_amd.eigen import _operands, jdsym, lobpcg
    assert jdsym._Operator is _operands._Operator and lobpcg._Operator is _operands._Operator


def test_new_symbols_are_declared_and_exported():
    from pysparse_amd import _capi
    for name in ("psp_bv_gram", "psp_bv_resid", "psp_lobpcg", "psp_debug_gen_ritz"):
        assert name in _capi.SYMBOLS and getattr(lib(), name).argtypes is not None


def small_matrix(n=30):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, n)
    for i in range(n):
        A[i, i] = i + 1.0
    return A


class Shape(object):
    def __init__(self, n):
        self.shape = (n, n)

    def matvec(self, x, y):
        y[:] = x

    precon = matvec


def call(A=None, M=None, K=None, **kw):
    from pysparse.eigen import lobpcg
    args = dict(k=2, tol=1e-8, itmax=10)
    args.update(kw)
    return lobpcg.lobpcg(A if A is not None else small_matrix(), M, K, **args)


@pytest.mark.parametrize("kw", [
    dict(k=0), dict(k=-1), dict(k=33), dict(k=11),                               # k out of range, 3 k > n
    dict(tol=0.0), dict(tol=-1e-8), dict(itmax=-1),
    dict(M=Shape(29)), dict(K=Shape(31)),                                        # shapes that differ
    dict(X0=np.zeros(29)), dict(X0=np.zeros((31, 2))), dict(X0=np.zeros((30, 3))),  # wrong length, more columns than k
    dict(X0=np.zeros(30, dtype=np.float32)), dict(X0=np.zeros((30, 2, 1))), dict(X0=[0.0] * 30),
    dict(X0=np.zeros((30, 0))),
], ids=lambda kw: ",".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_bad_arguments_raise_value_error_without_a_device(kw):
    with pytest.raises(ValueError):
        call(**kw)


def test_an_object_without_a_shape_or_a_method():
    with pytest.raises(ValueError):
        call(A=object())

    class NoMatvec(object):
        shape = (30, 30)

    with pytest.raises(TypeError):
        call(A=NoMatvec())


def test_messages():
    with pytest.raises(ValueError, match="shapes differ"):
        call(K=Shape(31))
    with pytest.raises(ValueError, match="X0 is not of correct type or shape"):
        call(X0=np.zeros(29))
    with pytest.raises(ValueError, match="3 k"):
        call(k=11)


def test_valid_call_without_a_device_reports_no_hip_device():
    from pysparse_amd import device
    for A in (small_matrix(), Shape(30)):  # native handle; duck-typed operator (its callback operator needs the device too)
        try:
            got = call(A=A)
        except Exception as e:  # noqa: B902
            got = e
        if device.device_count() > 0:
            assert isinstance(got, tuple) and len(got) == 4
        else:
            assert isinstance(got, Exception) and not isinstance(got, ValueError) and "no HIP device" in str(got)


def test_c_abi_validates_without_a_device():
    """psp_lobpcg answers PSP_EINVAL for a missing operator or a size out of range before it looks for a device"""
    L = lib()
    buf = np.zeros(64)
    kconv, it = C.c_int(), C.c_int()
    rc = L.psp_lobpcg(None, None, None, 30, 2, 1e-8, 10, None, 0, 0, buf.ctypes.data, buf.ctypes.data, 30,
                      buf.ctypes.data, C.byref(kconv), C.byref(it))
    assert rc == -1 and b"NULL" in L.psp_last_error()
    slot = np.zeros(4, dtype=np.int32)
    assert L.psp_bv_resid(8, 33, buf.ctypes.data, 8, buf.ctypes.data, 8, buf.ctypes.data, slot.ctypes.data,
                          buf.ctypes.data, 8, buf.ctypes.data) == -1
    assert L.psp_bv_gram(8, 2, buf.ctypes.data, 7, 2, buf.ctypes.data, 8, buf.ctypes.data, 2) == -1
