"""GPU: pysparse.eigen.jdsym -- the block-vector kernels through the C ABI (psp_bv_tdot / psp_bv_gemv / psp_bv_rotate)
against extended-precision NumPy, and the Jacobi-Davidson eigensolver against dense NumPy spectra on the same matrices
(or the analytic spectrum of the Poisson operator).

Bounds.  tdot: the project's dot-product bound 4 sqrt(n) eps ||V_c|| ||x||.  gemv / rotate: m products and m + 2 further
roundings at unit roundoff eps / 2 each, so (m + 2) eps (|beta y_i| + |alpha| sum_c |V_ic h_c|) covers them twice.
Solver: a pair was accepted with ||A q - lambda M q|| < jdtol, the factor 2 covers the recomputation; for a symmetric
pencil the eigenvalue error is bounded by the residual; iterated classical Gram-Schmidt leaves O(eps) orthogonality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def lib():
    from pysparse_amd import _capi
    return _capi.lib()


def buf(a):
    from pysparse_amd import device
    return device.DeviceBuffer.from_host(np.ascontiguousarray(a, dtype=np.float64))


def block(rng, n, m, ld):
    """column-major n x m block of leading dimension ld, padding rows NaN: (flat storage, n x m view of the values)"""
    store = np.full((max(m, 1), ld), np.nan)
    store[:m, :n] = rng.standard_normal((m, n))
    return store, store[:m, :n].T


NS = [1, 63, 64, 65, 1023, 4097, 65539]
MS = [1, 2, 7, 25, 33, 70]


def lds(n):
    return [n, n + 5, n + 6]  # tight; odd / even padding (8- and 16-byte column starts)


@pytest.mark.parametrize("n", NS)
def test_tdot(n):
    L = lib()
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    dx = buf(x)
    worst = 0.0
    for m in MS:
        for ld in lds(n):
            store, V = block(rng, n, m, ld)
            dV, dh = buf(store), buf(np.full(m + 1, np.nan))
            assert L.psp_bv_tdot(n, m, dV.ptr, ld, dx.ptr, dh.ptr) == 0, L.psp_last_error()
            h = dh.download()
            assert L.psp_bv_tdot(n, m, dV.ptr, ld, dx.ptr, dh.ptr) == 0
            assert np.array_equal(h, dh.download(), equal_nan=True), "two runs differ"
            assert np.isnan(h[m])  # nothing written behind the m results
            ref = (V.astype(LD).T @ x.astype(LD)).astype(np.float64)
            bound = 4 * np.sqrt(n) * EPS * np.linalg.norm(V, axis=0) * np.linalg.norm(x)
            err = np.abs(h[:m] - ref)
            worst = max(worst, (err / bound).max())
            assert np.all(err <= bound), (n, m, ld, (err / bound).max())
    print("tdot n=%d: worst error / bound %.3f" % (n, worst))


@pytest.mark.parametrize("n", [131073, 131074, 1 << 20])
def test_tdot_two_level_fold(n):
    """more than 256 workgroup sums per column (n > 256 * 512): the finishing block runs with 1024 threads, one wave per
    group of 256 sums, then wave 0 over the group sums -- the path every realistically sized problem takes"""
    L = lib()
    assert (n + 511) // 512 > 256
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    dx = buf(x)
    for m, ld in ((1, n), (9, n + 5), (9, n + 6), (17, n)):
        store, V = block(rng, n, m, ld)
        dV, dh = buf(store), buf(np.full(m + 1, np.nan))
        assert L.psp_bv_tdot(n, m, dV.ptr, ld, dx.ptr, dh.ptr) == 0, L.psp_last_error()
        h = dh.download()
        assert L.psp_bv_tdot(n, m, dV.ptr, ld, dx.ptr, dh.ptr) == 0
        assert np.array_equal(h, dh.download(), equal_nan=True), "two runs differ"
        assert np.isnan(h[m])
        ref = (V.astype(LD).T @ x.astype(LD)).astype(np.float64)
        bound = 4 * np.sqrt(n) * EPS * np.linalg.norm(V, axis=0) * np.linalg.norm(x)
        err = np.abs(h[:m] - ref)
        print("tdot n=%d m=%d ld=%d: worst error / bound %.4f" % (n, m, ld, (err / bound).max()))
        assert np.all(err <= bound), (n, m, ld)


@pytest.mark.parametrize("n", NS)
def test_gemv(n):
    L = lib()
    rng = np.random.default_rng(1000 + n)
    worst = 0.0
    for m in MS:
        for ld in lds(n):
            store, V = block(rng, n, m, ld)
            h = rng.standard_normal(m)
            y0 = rng.standard_normal(n)
            dV, dh = buf(store), buf(h)
            sabs = np.abs(V) @ np.abs(h)
            s = (V.astype(LD) @ h.astype(LD))
            for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.75, -1.5)):
                dy = buf(np.full(n, np.nan) if beta == 0.0 else y0)
                assert L.psp_bv_gemv(n, m, dV.ptr, ld, dh.ptr, alpha, beta, dy.ptr) == 0, L.psp_last_error()
                y = dy.download()
                ref = ((beta * y0.astype(LD) if beta != 0.0 else 0) + alpha * s).astype(np.float64)
                bound = (m + 2) * EPS * ((np.abs(beta * y0) if beta != 0.0 else 0) + abs(alpha) * sabs)
                err = np.abs(y - ref)
                assert np.all(np.isfinite(y)), (n, m, ld, alpha, beta)
                worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
                assert np.all(err <= bound), (n, m, ld, alpha, beta)
                dy2 = buf(np.full(n, np.nan) if beta == 0.0 else y0)
                assert L.psp_bv_gemv(n, m, dV.ptr, ld, dh.ptr, alpha, beta, dy2.ptr) == 0
                assert np.array_equal(y, dy2.download()), "two runs differ"
    print("gemv n=%d: worst error / bound %.3f" % (n, worst))


@pytest.mark.parametrize("n", NS)
def test_rotate(n):
    L = lib()
    rng = np.random.default_rng(2000 + n)
    worst = 0.0
    for j in MS + [128]:
        shapes = [(0, 0, max(j // 2, j - 15 if j > 15 else 0))]
        if j >= 4:
            shapes.append((2, 3, j - 3))
        for ld in lds(n):
            for dst0, u0, jn in shapes:
                store, V = block(rng, n, j, ld)
                ldu = j + 2
                Ust = np.full((j, ldu), np.nan)
                Ust[:, :j] = rng.standard_normal((j, j))  # Ust[c, r] = U[r, c]
                U = Ust[:, :j].T
                dV = buf(store)
                assert L.psp_bv_rotate(n, j, dV.ptr, ld, Ust.ctypes.data, ldu, u0, jn, dst0) == 0, L.psp_last_error()
                kept = Ust.copy()
                Ust[:] = np.nan  # U is borrowed for the call only: the caller may overwrite it at once (jdsym does)
                out = dV.download().reshape(store.shape)
                Ust[:] = kept
                Uc = U[:, u0:u0 + jn]
                ref = (V.astype(LD) @ Uc.astype(LD)).astype(np.float64)
                bound = (j + 2) * EPS * (np.abs(V) @ np.abs(Uc))
                got = out[dst0:dst0 + jn, :n].T
                err = np.abs(got - ref)
                if jn:
                    worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
                assert np.all(err <= bound), (n, j, ld, dst0, u0, jn)
                untouched = np.ones(store.shape, dtype=bool)
                untouched[dst0:dst0 + jn, :n] = False
                assert np.array_equal(out[untouched], store[untouched], equal_nan=True), "wrote outside the destination"
                dV2 = buf(store)
                assert L.psp_bv_rotate(n, j, dV2.ptr, ld, Ust.ctypes.data, ldu, u0, jn, dst0) == 0
                assert np.array_equal(out, dV2.download().reshape(store.shape), equal_nan=True), "two runs differ"
    print("rotate n=%d: worst error / bound %.3f" % (n, worst))


def test_no_columns_is_a_no_op():
    L = lib()
    n = 1023
    rng = np.random.default_rng(5)
    y0 = rng.standard_normal(n)
    dV, dx, dh, dy = buf(np.zeros(8)), buf(y0), buf(np.full(4, np.nan)), buf(y0)
    assert L.psp_bv_tdot(n, 0, dV.ptr, n, dx.ptr, dh.ptr) == 0
    assert np.all(np.isnan(dh.download()))
    assert L.psp_bv_gemv(n, 0, dV.ptr, n, dh.ptr, -1.0, 1.0, dy.ptr) == 0
    assert np.array_equal(dy.download(), y0)
    assert L.psp_bv_gemv(n, 0, None, n, None, 1.0, 2.0, dy.ptr) == 0
    assert np.array_equal(dy.download(), 2.0 * y0)
    dn = buf(np.full(n, np.nan))
    assert L.psp_bv_gemv(n, 0, None, n, None, 1.0, 0.0, dn.ptr) == 0
    assert np.array_equal(dn.download(), np.zeros(n))
    assert L.psp_bv_rotate(n, 0, dy.ptr, n, None, 1, 0, 0, 0) == 0
    assert L.psp_bv_rotate(n, 129, dy.ptr, n, y0.ctypes.data, 129, 0, 1, 0) != 0  # j beyond 128: refused, not truncated


# ====================================================================== the solver

def tridiag(d, e):
    n = len(d)
    return np.diag(np.asarray(d, dtype=float)) + np.diag(np.full(n - 1, e), 1) + np.diag(np.full(n - 1, e), -1)


T300 = tridiag(np.arange(1.0, 301.0), 0.1)
M300 = tridiag(1.0 + 0.5 * (np.arange(300) % 3), 0.05)


def ll(dense):
    from pysparse.sparse import spmatrix
    n = dense.shape[0]
    A = spmatrix.ll_mat(n, n)
    for i, c in zip(*np.nonzero(dense)):
        A[int(i), int(c)] = float(dense[i, c])
    return A


def pencil_spectrum(A, M=None):
    if M is None:
        return np.linalg.eigvalsh(A)
    Lc = np.linalg.cholesky(M)
    B = np.linalg.solve(Lc, np.linalg.solve(Lc, A).T).T
    return np.linalg.eigvalsh((B + B.T) / 2)


def poisson_spectrum(nx, ny):
    p, q = np.arange(1, nx + 1), np.arange(1, ny + 1)
    return np.sort((4 - 2 * np.cos(p * np.pi / (nx + 1)))[:, None] - 2 * np.cos(q * np.pi / (ny + 1))[None, :], axis=None)


def nearest(spec, tau, k):
    return np.sort(spec[np.argsort(np.abs(spec - tau), kind="stable")[:k]])


def check_pairs(res, apply_a, apply_m, spec, jdtol):
    """the three assertions every returned pair must satisfy"""
    kconv, lam, Q, it, it_inner = res
    assert lam.shape == (kconv,) and Q.shape[1] == kconv and Q.flags.c_contiguous and Q.dtype == np.float64
    if kconv == 0:
        return
    MQ = apply_m(Q)
    R = apply_a(Q) - MQ * lam
    resid = np.linalg.norm(R, axis=0)
    dist = np.abs(lam[:, None] - spec[None, :]).min(axis=1)
    orth = np.abs(Q.T @ MQ - np.eye(kconv)).max()
    print("kconv %d it %d it_inner %d: max residual %.3e, eigenvalue error %.3e, orthogonality %.3e"
          % (kconv, it, it_inner, resid.max(), dist.max(), orth))
    assert np.all(resid <= 2 * jdtol)
    assert np.all(dist <= 2 * jdtol)
    assert orth <= 1e-10


def check_nearest(res, spec, tau, kmax, jdtol):
    assert res[0] == kmax
    assert np.abs(np.sort(res[1]) - nearest(spec, tau, kmax)).max() <= 2 * jdtol, (np.sort(res[1]), nearest(spec, tau, kmax))


def dense_ops(A, M=None):
    return (lambda Q: A @ Q), ((lambda Q: M @ Q) if M is not None else (lambda Q: Q))


def run(A, M=None, K=None, kmax=4, tau=0.0, jdtol=1e-8, itmax=400, linsolver=None, **kw):
    from pysparse.eigen import jdsym
    from pysparse.itsolvers import krylov
    return jdsym.jdsym(A, M, K, kmax, tau, jdtol, itmax, linsolver or krylov.qmrs, **kw)


@pytest.fixture(scope="module")
def t300():
    A = ll(T300)
    return {"ll": A, "csr": A.to_csr(), "sss": A.to_sss(), "spec": np.linalg.eigvalsh(T300)}


@pytest.fixture(scope="module")
def m300():
    Mm = ll(M300)
    return {"csr": Mm.to_csr(), "sss": Mm.to_sss(), "spec": pencil_spectrum(T300, M300)}


def test_diag3():
    res = run(ll(np.diag([1.0, 2.0, 3.0])), kmax=3, tau=1.0, jdtol=1e-9, itmax=100)
    kconv, lam, Q, it, it_inner = res
    assert kconv == 3
    assert np.abs(np.sort(lam) - [1.0, 2.0, 3.0]).max() <= 2e-9
    P = np.abs(Q[:, np.argsort(lam)])
    assert np.abs(P - np.eye(3)).max() <= 1e-8
    check_pairs(res, *dense_ops(np.diag([1.0, 2.0, 3.0])), spec=np.array([1.0, 2.0, 3.0]), jdtol=1e-9)


@pytest.mark.parametrize("solver", ["qmrs", "minres", "cgs", "bicgstab", "gmres"])
def test_t300_solvers(t300, solver):
    from pysparse.itsolvers import krylov
    res = run(t300["csr"], linsolver=getattr(krylov, solver))
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 0.0, 4, 1e-8)


def test_t300_pcg(t300):
    """the projected operator need not suit CG: every returned pair is valid, completeness is not asserted"""
    from pysparse.itsolvers import krylov
    res = run(t300["csr"], linsolver=krylov.pcg)
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    assert res[0] >= 1


def test_restart_and_determinism(t300):
    res = run(t300["csr"], jmax=6, jmin=3)
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 0.0, 4, 1e-8)
    again = run(t300["csr"], jmax=6, jmin=3)
    assert res[0] == again[0] and res[3:] == again[3:]
    assert np.array_equal(res[1], again[1]) and np.array_equal(res[2], again[2])


def test_interior(t300):
    res = run(t300["csr"], kmax=3, tau=100.4)
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 100.4, 3, 1e-8)


@pytest.mark.parametrize("optype", [1, 2])
@pytest.mark.parametrize("mform", ["csr", "sss"])
def test_generalised(t300, m300, mform, optype):
    res = run(t300["csr"], M=m300[mform], optype=optype)
    check_pairs(res, *dense_ops(T300, M300), spec=m300["spec"], jdtol=1e-8)
    check_nearest(res, m300["spec"], 0.0, 4, 1e-8)


class CountingJacobi(object):
    """duck-typed preconditioner: shape + precon on NumPy arrays"""

    def __init__(self, dense):
        self.shape = dense.shape
        self.dinv = 1.0 / np.diag(dense)
        self.calls = 0

    def precon(self, x, y):
        self.calls += 1
        y[:] = x * self.dinv


@pytest.mark.parametrize("optype", [1, 2])
@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kind", ["jacobi", "ssor", "python"])
def test_preconditioned(t300, m300, kind, mass, optype):
    from pysparse.precon import precon
    counter = None
    if kind == "jacobi":
        K = precon.jacobi(t300["csr"])
    elif kind == "ssor":
        K = precon.ssor(t300["sss"])
    else:
        K = counter = CountingJacobi(T300)
    M = m300["csr"] if mass else None
    spec = m300["spec"] if mass else t300["spec"]
    res = run(t300["csr"], M=M, K=K, optype=optype)
    check_pairs(res, *dense_ops(T300, M300 if mass else None), spec=spec, jdtol=1e-8)
    check_nearest(res, spec, 0.0, 4, 1e-8)
    plain = run(t300["csr"], M=M, optype=optype)
    print("%s, M %s, optype %d: it_inner %d with K, %d without" % (kind, mass, optype, res[4], plain[4]))
    if counter is not None:
        assert counter.calls > 0


@pytest.mark.parametrize("form", ["csr", "sss"])
def test_poisson(form):
    from pysparse.sparse import spmatrix
    P = spmatrix.poisson_csr(24, 17) if form == "csr" else spmatrix.poisson_sss(24, 17)
    spec = poisson_spectrum(24, 17)

    def apply_a(Q):
        out = np.empty_like(Q)
        for c in range(Q.shape[1]):
            x, y = np.ascontiguousarray(Q[:, c]), np.empty(Q.shape[0])
            P.matvec(x, y)
            out[:, c] = y
        return out
    res = run(P, kmax=5)
    check_pairs(res, apply_a, lambda Q: Q, spec=spec, jdtol=1e-8)
    check_nearest(res, spec, 0.0, 5, 1e-8)


@pytest.mark.parametrize("blkwise", [0, 1])
def test_block(blkwise):
    """the block variant may converge a slightly farther eigenvalue before a nearer one: the four values lie among the
    eight nearest tau and the smallest one is among them"""
    from pysparse.sparse import spmatrix
    P = spmatrix.poisson_csr(24, 17)
    spec = poisson_spectrum(24, 17)

    def apply_a(Q):
        out = np.empty_like(Q)
        for c in range(Q.shape[1]):
            x, y = np.ascontiguousarray(Q[:, c]), np.empty(Q.shape[0])
            P.matvec(x, y)
            out[:, c] = y
        return out
    res = run(P, kmax=4, blksize=2, blkwise=blkwise, jmin=10)
    check_pairs(res, apply_a, lambda Q: Q, spec=spec, jdtol=1e-8)
    assert res[0] == 4
    eight = nearest(spec, 0.0, 8)
    lam = np.sort(res[1])
    print("block blkwise %d: lambda %s" % (blkwise, lam))
    assert np.all(np.abs(lam[:, None] - eight[None, :]).min(axis=1) <= 2e-8)
    assert abs(lam[0] - spec[0]) <= 2e-8
    assert np.all(np.diff(lam) > 1e-6)  # four different pairs


@pytest.mark.parametrize("layout", ["C", "F", "1d"])
def test_v0_exact_vectors_converge_without_a_solve(t300, layout):
    w, X = np.linalg.eigh(T300)
    if layout == "1d":
        V0, kmax = np.ascontiguousarray(X[:, 0]), 1
    else:
        V0, kmax = np.array(X[:, :4], order=layout), 4
        assert V0.flags.c_contiguous == (layout == "C")
    res = run(t300["csr"], kmax=kmax, V0=V0)
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 0.0, kmax, 1e-8)
    assert res[3] == 0 and res[4] == 0


def test_projector():
    Z = np.zeros((300, 300))
    big = np.block([[T300 + 50.0 * np.eye(300), Z], [Z, T300]])
    calls = []

    def project(x):
        calls.append(1)
        x[300:] = 0.0
    res = run(ll(big).to_csr(), kmax=3, projector=project)
    spec = np.linalg.eigvalsh(big)
    check_pairs(res, *dense_ops(big), spec=spec, jdtol=1e-8)
    assert res[0] == 3 and calls
    assert np.abs(np.sort(res[1]) - np.linalg.eigvalsh(T300 + 50.0 * np.eye(300))[:3]).max() <= 2e-8
    assert np.abs(res[2][300:]).max() <= 1e-12


def test_duck_typed_matrix(t300):
    class Matrix(object):
        shape = (300, 300)
        calls = 0

        def matvec(self, x, y):
            Matrix.calls += 1
            y[:] = T300 @ x
    res = run(Matrix())
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 0.0, 4, 1e-8)
    assert Matrix.calls > 0


def test_foreign_solver(t300):
    from pysparse.itsolvers import krylov
    seen = []

    def solver(A, b, x, tol, maxit, K):
        seen.append(A.shape)
        assert callable(A.matvec) and callable(A.precon) and callable(K.precon)
        assert b.shape == (300,) and x.shape == (300,) and not x.any()
        return krylov.qmrs(A, b, x, tol, maxit, K)
    res = run(t300["csr"], linsolver=solver)
    check_pairs(res, *dense_ops(T300), spec=t300["spec"], jdtol=1e-8)
    check_nearest(res, t300["spec"], 0.0, 4, 1e-8)
    assert seen and set(seen) == {(300, 300)}


def test_exception_in_a_callback_reaches_the_caller(t300):
    def solver(A, b, x, tol, maxit, K):
        raise KeyError("from the linear solver")
    with pytest.raises(KeyError, match="from the linear solver"):
        run(t300["csr"], linsolver=solver)


def test_useless_corrections_are_replaced():
    """a linear solver that returns x = 0 gives no direction: the search space is extended with pseudo-random vectors
    instead (the reference divides by zero); on diag(1 .. 6) the space is complete at j = 6 and the pairs are exact"""
    D = np.diag(np.arange(1.0, 7.0))
    calls = []

    def solver(A, b, x, tol, maxit, K):
        calls.append(1)
        x[:] = 0.0
        return 0, 1, 0.0
    res = run(ll(D), kmax=2, itmax=50, linsolver=solver)
    check_pairs(res, *dense_ops(D), spec=np.arange(1.0, 7.0), jdtol=1e-8)
    check_nearest(res, np.arange(1.0, 7.0), 0.0, 2, 1e-8)
    assert calls


def test_budget(t300):
    kconv, lam, Q, it, it_inner = run(t300["csr"], itmax=2)
    assert it == 2 and kconv < 4
    assert lam.shape == (kconv,) and Q.shape == (300, kconv)


def test_multi_device_matrix_is_refused():
    from pysparse.sparse import spmatrix
    with pytest.raises(ValueError):
        run(spmatrix.poisson_csr(24, 17, devices=[0, 0]), kmax=2)


def test_scale():
    """n = 65 536: grids of 128 workgroups per kernel; the two-level fold of the block dot product starts beyond
    n = 131 072 (test_tdot_two_level_fold)"""
    from pysparse.sparse import spmatrix
    P = spmatrix.poisson_csr(256, 256)
    spec = poisson_spectrum(256, 256)

    def apply_a(Q):
        out = np.empty_like(Q)
        for c in range(Q.shape[1]):
            x, y = np.ascontiguousarray(Q[:, c]), np.empty(Q.shape[0])
            P.matvec(x, y)
            out[:, c] = y
        return out
    res = run(P, kmax=2)
    check_pairs(res, apply_a, lambda Q: Q, spec=spec, jdtol=1e-8)
    check_nearest(res, spec, 0.0, 2, 1e-8)
