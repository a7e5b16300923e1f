"""CPU: the host side of pysparse.eigen.jdsym -- the small dense algebra behind the eigensolver (projected eigenproblem
by cyclic Jacobi rotations, the ordering of the Ritz pairs, LU with partial pivoting) through the library's test hooks,
and the import / signature / argument validation of the Python surface.  Nothing here needs a GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
ORDERS = [1, 2, 3, 10, 25, 64, 128]


def lib():
    from pysparse_amd import _capi
    return _capi.lib()


def ritz(Mfull, tau=0.0, strategy=0, ldm=None, ldu=None):
    """psp_debug_ritz on the upper triangle of Mfull; the strict lower triangle is handed over as NaN"""
    j = Mfull.shape[0]
    ldm = ldm or j
    ldu = ldu or j
    buf = np.full((j, ldm), np.nan)  # column-major: buf[c, r] = M[r, c]
    for c in range(j):
        buf[c, :c + 1] = Mfull[:c + 1, c]
    s = np.empty(j)
    U = np.full((j, ldu), np.nan)
    rc = lib().psp_debug_ritz(j, buf.ctypes.data, ldm, float(tau), strategy, s.ctypes.data, U.ctypes.data, ldu)
    assert rc == 0, lib().psp_last_error()
    return s, U[:, :j].T.copy()  # U[:, i] = eigenvector i


def symmetric(kind, j, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        B = rng.standard_normal((j, j))
        return (B + B.T) / 2
    if kind == "diagonal":
        return np.diag(rng.standard_normal(j) * 10.0)
    # repeated eigenvalues: an orthogonal similarity of a diagonal with clusters of equal entries
    d = np.repeat(rng.standard_normal((j + 2) // 3), 3)[:j]
    Qm, _ = np.linalg.qr(rng.standard_normal((j, j)))
    S = Qm @ np.diag(d) @ Qm.T
    return (S + S.T) / 2


@pytest.mark.parametrize("kind", ["random", "diagonal", "repeated"])
@pytest.mark.parametrize("j", ORDERS)
def test_ritz_eigenpairs(j, kind):
    Mf = symmetric(kind, j, 100 * j + len(kind))
    fro = np.linalg.norm(Mf)
    s, U = ritz(Mf, ldm=j + 3, ldu=j + 1)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U))
    exact = np.linalg.eigvalsh(Mf)
    err = np.abs(np.sort(s) - exact).max()
    orth = np.abs(U.T @ U - np.eye(j)).max()
    res = np.abs(Mf @ U - U * s).max()
    print("j=%d %s: eigenvalue error %.3e (bound %.3e), orthogonality %.3e, residual %.3e"
          % (j, kind, err, 100 * j * EPS * fro, orth, res))
    assert err <= 100 * j * EPS * fro
    assert orth <= 100 * j * EPS
    assert res <= 100 * j * EPS * fro
    assert np.all(np.diff(np.abs(s)) >= 0)  # tau = 0, strategy 0: ascending |s|


def test_ritz_reads_only_the_upper_triangle():
    Mf = symmetric("random", 10, 7)
    s1, _ = ritz(Mf)
    buf = np.triu(Mf).T.copy() + np.tril(np.full((10, 10), 1e300), -1).T  # another lower triangle, column-major
    s2, U2 = np.empty(10), np.empty((10, 10))
    assert lib().psp_debug_ritz(10, buf.ctypes.data, 10, 0.0, 0, s2.ctypes.data, U2.ctypes.data, 10) == 0
    assert np.array_equal(s1, s2)


def test_sorteig_order():
    vals = np.array([-3.0, -1.0, 0.5, 1.0, 2.0, 3.0, 4.5, 7.0])  # tau = 1: 1.0 sits on it, (-1, 3) and (0.5 .. ) tie
    Mf = np.diag(vals)
    tau = 1.0
    s0, U0 = ritz(Mf, tau, 0)
    # ascending |s - tau|; of an equidistant pair the smaller value first
    assert s0.tolist() == [1.0, 0.5, 2.0, -1.0, 3.0, 4.5, -3.0, 7.0]
    assert np.all(np.diff(np.abs(s0 - tau)) >= 0)
    for i, v in enumerate(s0):  # the vectors moved with their values
        assert abs(abs(U0[list(vals).index(v), i]) - 1.0) <= 8 * EPS
    s1, U1 = ritz(Mf, tau, 1)
    # everything below tau goes behind the others (there: ascending value); a value exactly at tau is not below it
    assert s1.tolist() == [1.0, 2.0, 3.0, 4.5, 7.0, -3.0, -1.0, 0.5]
    for i, v in enumerate(s1):
        assert abs(abs(U1[list(vals).index(v), i]) - 1.0) <= 8 * EPS
    # a dense matrix: same rules
    rng = np.random.default_rng(3)
    Qm, _ = np.linalg.qr(rng.standard_normal((8, 8)))
    D = Qm @ Mf @ Qm.T
    D = (D + D.T) / 2
    s2, _ = ritz(D, tau, 1)
    below = s2 < tau
    first_below = int(np.argmax(below)) if below.any() else len(s2)
    assert not below[:first_below].any() and below[first_below:].all()
    assert np.all(np.diff(np.abs(s2[:first_below] - tau)) >= 0)


def test_ritz_rejects_bad_arguments():
    a = np.zeros(4)
    assert lib().psp_debug_ritz(0, a.ctypes.data, 1, 0.0, 0, a.ctypes.data, a.ctypes.data, 1) != 0
    assert lib().psp_debug_ritz(129, a.ctypes.data, 129, 0.0, 0, a.ctypes.data, a.ctypes.data, 129) != 0
    assert lib().psp_debug_ritz(2, a.ctypes.data, 2, 0.0, 2, a.ctypes.data, a.ctypes.data, 2) != 0


def lu_solve(Hm, w, ldh=None):
    k = Hm.shape[0]
    ldh = ldh or k
    buf = np.full((k, ldh), np.nan)
    buf[:, :k] = Hm.T
    piv = np.zeros(k, dtype=np.int32)
    assert lib().psp_debug_lu_factor(k, buf.ctypes.data, ldh, piv.ctypes.data) == 0, lib().psp_last_error()
    x = np.array(w, dtype=np.float64)
    assert lib().psp_debug_lu_solve(k, buf.ctypes.data, ldh, piv.ctypes.data, x.ctypes.data) == 0
    return x, piv


@pytest.mark.parametrize("k", [1, 2, 5, 20])
def test_lu_against_numpy(k):
    rng = np.random.default_rng(k)
    for trial in range(4):
        Hm = rng.standard_normal((k, k))
        if trial == 1:
            Hm[0, 0] = 0.0 if k > 1 else 2.0  # a zero where the first pivot would be taken without pivoting
        w = rng.standard_normal(k)
        x, _ = lu_solve(Hm, w, ldh=k + trial)
        ref = np.linalg.solve(Hm, w)
        cond = np.linalg.cond(Hm)
        err = np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300)
        print("k=%d trial %d: relative error %.3e, bound %.3e" % (k, trial, err, 100 * k * EPS * cond))
        assert err <= 100 * k * EPS * cond


def test_lu_needs_the_pivot():
    x, piv = lu_solve(np.array([[0.0, 1.0], [1.0, 0.0]]), [3.0, 5.0])
    assert x.tolist() == [5.0, 3.0]
    assert piv[0] == 1
    Hs = np.zeros((2, 2))
    piv = np.zeros(2, dtype=np.int32)
    assert lib().psp_debug_lu_factor(2, Hs.ctypes.data, 2, piv.ctypes.data) != 0  # singular: reported, not divided by


# ---------------------------------------------------------------------- the Python surface

KEYWORDS = ["A", "M", "K", "kmax", "tau", "jdtol", "itmax", "linsolver", "jmax", "jmin", "blksize", "blkwise", "V0",
            "optype", "linitmax", "eps_tr", "toldecay", "clvl", "strategy", "projector"]


def test_import_and_signature():
    from pysparse.eigen import jdsym
    import pysparse.eigen.jdsym as mod
    assert mod is jdsym and callable(jdsym.jdsym)
    sig = inspect.signature(jdsym.jdsym)
    assert list(sig.parameters) == KEYWORDS
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(jmax=25, jmin=10, blksize=1, blkwise=0, V0=None, optype=2, linitmax=200, eps_tr=1e-3,
                            toldecay=1.5, clvl=0, strategy=0, projector=None)


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
    from pysparse.eigen import jdsym
    from pysparse.itsolvers import krylov
    args = dict(kmax=2, tau=0.0, jdtol=1e-8, itmax=10, linsolver=krylov.qmrs)
    args.update(kw)
    return jdsym.jdsym(A if A is not None else small_matrix(), M, K, **args)


@pytest.mark.parametrize("kw", [
    dict(M=Shape(29)), dict(K=Shape(31)), dict(projector=Shape(7)),        # shape mismatch
    dict(jmin=25, jmax=25), dict(jmin=26, jmax=25), dict(jmin=0),          # jmin >= jmax, jmin < 1
    dict(kmax=31), dict(kmax=0),                                           # kmax > n
    dict(blksize=11, kmax=12),                                             # blksize > jmin
    dict(blksize=3, kmax=3, jmin=23),                                      # blksize > jmax - jmin
    dict(blksize=3, kmax=2),                                               # blksize > kmax
    dict(toldecay=1.0), dict(toldecay=0.5),                                # toldecay <= 1
    dict(jdtol=0.0), dict(jdtol=-1e-8),                                    # jdtol <= 0
    dict(optype=0), dict(optype=3),                                        # bad optype
    dict(blkwise=2), dict(strategy=2), dict(eps_tr=-1.0), dict(itmax=-1), dict(linitmax=-1),
    dict(V0=np.zeros(29)), dict(V0=np.zeros((31, 2))), dict(V0=np.zeros(30, dtype=np.float32)),
    dict(V0=np.zeros((30, 2, 1))), dict(V0=[0.0] * 30),                    # V0 of wrong length, dtype, rank, type
], ids=lambda kw: ",".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_bad_arguments_raise_value_error_without_a_device(kw):
    with pytest.raises(ValueError):
        call(**kw)


def test_reference_messages():
    with pytest.raises(ValueError, match="matrix, preconditioner or projector shapes differ"):
        call(K=Shape(31))
    with pytest.raises(ValueError, match="V0 is not of correct type or shape"):
        call(V0=np.zeros(29))


def outcome(**kw):
    """a valid call: the result where a GPU is present, else the exception it raised"""
    try:
        return call(**kw)
    except Exception as e:  # noqa: B902
        return e


def test_clamping_accepts_the_defaults_on_a_tiny_matrix():
    """n = 3 with jmax = 25, jmin = 10 is valid (jmax -> 3, jmin -> 2): whatever fails afterwards is not a ValueError"""
    from pysparse_amd import device
    got = outcome(A=small_matrix(3), kmax=3)
    if device.device_count() > 0:
        assert got[0] == 3
    else:
        assert not isinstance(got, ValueError) and "no HIP device" in str(got)


def test_valid_call_without_a_device_reports_no_hip_device():
    from pysparse_amd import device
    for A in (small_matrix(), Shape(30)):  # native handle; duck-typed operator (its callback operator needs the device too)
        got = outcome(A=A)
        if device.device_count() > 0:
            assert isinstance(got, tuple) and len(got) == 5
        else:
            assert isinstance(got, Exception) and not isinstance(got, ValueError) and "no HIP device" in str(got)


def test_c_abi_validates_without_a_device():
    """psp_jdsym itself answers PSP_EINVAL for a missing operator before it looks for a device"""
    from pysparse_amd import _capi
    L = _capi.lib()
    p = _capi.JdsymParams()
    p.kmax, p.jmax, p.jmin, p.itmax, p.blksize, p.optype, p.linitmax = 2, 25, 10, 10, 1, 2, 200
    p.tau, p.jdtol, p.eps_tr, p.toldecay, p.linsolver = 0.0, 1e-8, 1e-3, 1.0, _capi.LIN_QMRS
    kconv, it, it_inner = C.c_int(), C.c_int(), C.c_int()
    buf = np.zeros(64)
    rc = L.psp_jdsym(None, None, None, 30, C.byref(p), C.byref(kconv), buf.ctypes.data, buf.ctypes.data, C.byref(it),
                     C.byref(it_inner))
    assert rc == -1 and b"NULL" in L.psp_last_error()
