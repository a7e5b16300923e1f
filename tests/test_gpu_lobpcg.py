"""GPU: pysparse.eigen.lobpcg (psp_lobpcg.hip) -- the k smallest eigenpairs of grid operators against the analytic
spectrum of the Poisson operator (or scipy.linalg.eigh of the dense matrix at n ~ 10^3).

Every case asserts (tol = 1e-8): the returned residuals are <= tol and the residuals recomputed on the host from the
returned lambda and Q are <= 2 tol (the factor covers the recomputation); Q' M Q - I <= 1e-12; lambda ascending;
eigenvalues within 2 tol / sqrt(lambda_min(M)) of the reference (for a symmetric pencil the eigenvalue error is bounded by
the residual in the M^-1 norm); two runs are bit-identical; `it` stays within its cap.

The caps on `it` are conditions: about three times what a NumPy LOBPCG of the same definition needed on the same operator
with the V-cycle oracles of tests/test_multigrid_host.py / tests/test_multigrid_galerkin_host.py as K (the device's
pseudo-random start differs from NumPy's, hence the factor).  The two counts measured for this file on the CPU:
33 x 31 with kappa = exp U(-1.5, 1.5) and the Galerkin oracle, k = 3: 15 iterations (cap 45); 363 x 362 Poisson with the
cycle oracle, k = 4: 19 iterations (cap 57)."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest
import scipy.linalg

import test_multigrid_galerkin_host as galerkin_host
from test_multigrid_host import grid_operator

pytestmark = pytest.mark.gpu

TOL = 1e-8


def poisson_spectrum(grid, count):
    lam = np.zeros(1)
    for m in grid:
        lam = (lam[:, None] + (2.0 - 2.0 * np.cos(np.pi * np.arange(1, m + 1) / (m + 1)))[None, :]).ravel()
    return np.sort(lam)[:count]


def native(grid, form="csr"):
    from pysparse.sparse import spmatrix
    if len(grid) == 1:  # the generators take two or three axes
        return ll_from(grid_operator(grid, (1.0,), 0.0)).to_csr()
    return (spmatrix.poisson_csr if form == "csr" else spmatrix.poisson_sss)(*grid)


def ll_from(S):
    from pysparse.sparse import spmatrix
    n = S.shape[0]
    L = spmatrix.ll_mat(n, n, S.nnz)
    Co = S.tocoo()
    for i, j, v in zip(Co.row, Co.col, Co.data):
        L[int(i), int(j)] = float(v)
    return L


def solve(A, M, K, k, itmax, X0=None):
    from pysparse.eigen import lobpcg
    return lobpcg.lobpcg(A, M, K, k, TOL, itmax, X0)


def check(S, Md, got, again, reference, cap):
    """S: the matrix (SciPy), Md: the diagonal of M or None"""
    lam, Q, res, it = got
    n, k = Q.shape
    print("n=%d k=%d: it=%d (cap %d), res max %.3e" % (n, k, it, cap, res.max()))
    assert Q.flags.c_contiguous and lam.shape == (k,) and res.shape == (k,)
    assert it <= cap, (it, cap)
    assert np.all(res <= TOL), res
    MQ = Q if Md is None else Md[:, None] * Q
    host = np.linalg.norm(S @ Q - MQ * lam, axis=0)
    assert np.all(host <= 2 * TOL), host
    assert np.abs(Q.T @ MQ - np.eye(k)).max() <= 1e-12
    assert np.all(np.diff(lam) >= 0)
    lmin = 1.0 if Md is None else Md.min()
    assert np.abs(lam - reference[:k]).max() <= 2 * TOL / np.sqrt(lmin), (lam, reference[:k])
    assert np.array_equal(lam, again[0]) and np.array_equal(Q, again[1]), "two runs differ"
    assert it == again[3]


def mg(A, grid, **kw):
    from pysparse.precon import precon
    return precon.multigrid(A, grid, **kw)


@pytest.mark.parametrize("form", ["csr", "sss"])
@pytest.mark.parametrize("k", [1, 3, 4, 6])
def test_poisson_2d_with_multigrid(k, form):
    grid = (33, 31)
    A = native(grid, form)
    K = mg(A, grid)
    check(grid_operator(grid, (1.0, 1.0), 0.0), None, solve(A, None, K, k, 70), solve(A, None, K, k, 70),
          poisson_spectrum(grid, k), 70)


def test_poisson_2d_without_a_preconditioner():
    grid = (33, 31)
    A = native(grid)
    check(grid_operator(grid, (1.0, 1.0), 0.0), None, solve(A, None, None, 4, 750), solve(A, None, None, 4, 750),
          poisson_spectrum(grid, 4), 750)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_poisson_3d_with_multigrid(k):
    grid = (12, 10, 9)
    A = native(grid)
    K = mg(A, grid)
    check(grid_operator(grid, (1.0, 1.0, 1.0), 0.0), None, solve(A, None, K, k, 75), solve(A, None, K, k, 75),
          poisson_spectrum(grid, k), 75)


@pytest.mark.parametrize("grid,k,cap", [((64,), 4, 45), ((40, 40), 3, 50), ((182, 181), 4, 60), ((363, 362), 4, 57),
                                        ((50, 54, 60), 4, 70)],
                         ids=["64", "40x40-double-eigenvalue", "182x181", "363x362-two-level-fold", "50x54x60"])
def test_poisson_grids_with_multigrid(grid, k, cap):
    A = native(grid)
    K = mg(A, grid)
    check(grid_operator(grid, (1.0,) * len(grid), 0.0), None, solve(A, None, K, k, cap), solve(A, None, K, k, cap),
          poisson_spectrum(grid, k), cap)


class Diagonal(object):
    """a mass matrix with only `shape` and `matvec`"""

    def __init__(self, d):
        self.d, self.shape = d, (d.size, d.size)

    def matvec(self, x, y):
        y[:] = self.d * x


def test_generalised_problem_with_a_diagonal_mass_matrix():
    grid = (33, 31)
    n = grid[0] * grid[1]
    d = np.exp(np.random.default_rng(5).uniform(-1.0, 1.0, n))
    S = grid_operator(grid, (1.0, 1.0), 0.0)
    reference = scipy.linalg.eigh(S.toarray(), np.diag(d), eigvals_only=True)
    A = native(grid)
    K = mg(A, grid)
    check(S, d, solve(A, Diagonal(d), K, 3, 45), solve(A, Diagonal(d), K, 3, 45), reference, 45)


def exp_uniform_operator(grid):
    """-div(kappa grad u) with kappa = exp U(-1.5, 1.5) per cell, assembled as the Galerkin tests assemble theirs"""
    def kappa(grid, kind, seed=0):
        shape = tuple(int(g) for g in grid)[::-1]
        return np.exp(np.random.default_rng([seed, len(grid)] + list(grid)).uniform(-1.5, 1.5, shape))
    with mock.patch.object(galerkin_host, "kappa_field", kappa):
        return galerkin_host.varying_operator(grid, "exp-uniform", 0.0)


@pytest.mark.parametrize("which,cap", [("jacobi", 500), ("galerkin", 45)])
def test_varying_coefficients(which, cap):
    from pysparse.precon import precon
    grid = (33, 31)
    S = exp_uniform_operator(grid)
    A = ll_from(S).to_csr()
    K = precon.jacobi(A, 1.0, 1) if which == "jacobi" else mg(A, grid, galerkin=True)
    reference = scipy.linalg.eigh(S.toarray(), eigvals_only=True)
    check(S, None, solve(A, None, K, 3, cap), solve(A, None, K, 3, cap), reference, cap)


class OnlyMatvec(object):
    def __init__(self, S):
        self.S, self.shape = S, S.shape

    def matvec(self, x, y):
        y[:] = self.S @ x


class OnlyPrecon(object):
    def __init__(self, K):
        self.K, self.shape = K, K.shape

    def precon(self, x, y):
        self.K.precon(x, y)


def test_python_operands_give_the_native_eigenpairs():
    grid = (33, 31)
    S = grid_operator(grid, (1.0, 1.0), 0.0)
    A = native(grid)
    K = mg(A, grid)
    lam, Q, res, it = solve(A, None, K, 3, 70)
    for a, kk in ((OnlyMatvec(S), K), (A, OnlyPrecon(K))):
        lam2, Q2, res2, it2 = solve(a, None, kk, 3, 70)
        assert np.all(res2 <= TOL)
        assert np.abs(lam2 - lam).max() <= 1e-7
        # lambda_2 and lambda_3 of the 33 x 31 grid are simple: the vectors agree up to sign
        signs = np.sign(np.sum(Q * Q2, axis=0))
        assert np.abs(Q2 * signs - Q).max() <= 1e-7


class Boom(Exception):
    pass


def test_an_exception_in_a_callback_reaches_the_caller():
    grid = (33, 31)
    A = native(grid)

    class Bad(object):
        shape = (grid[0] * grid[1],) * 2

        def precon(self, x, y):
            raise Boom("from the callback")

    with pytest.raises(Boom):
        solve(A, None, Bad(), 2, 10)


def test_a_full_start_block_is_used():
    grid = (33, 31)
    A = native(grid)
    K = mg(A, grid)
    lam, Q, res, it = solve(A, None, K, 3, 70)
    lam0, Q0, res0, it0 = solve(A, None, K, 3, 70, X0=Q)
    assert it0 == 0 and np.all(res0 <= TOL)
    assert np.abs(lam0 - lam).max() <= 1e-12
    lam1, Q1, res1, it1 = solve(A, None, K, 3, 70, X0=np.asfortranarray(Q))  # the strides do not matter
    assert it1 == 0 and np.array_equal(lam1, lam0) and np.array_equal(Q1, Q0)
    rough = Q + 1e-3 * np.random.default_rng(1).standard_normal(Q.shape)
    lam2, _, res2, it2 = solve(A, None, K, 3, 70, X0=rough)
    assert 0 < it2 <= it and np.all(res2 <= TOL) and np.abs(lam2 - lam).max() <= 2 * TOL


def test_itmax_reached_is_not_an_error():
    grid = (33, 31)
    A = native(grid)
    lam, Q, res, it = solve(A, None, mg(A, grid), 4, 2)
    assert it == 2
    assert int(np.sum(res <= TOL)) < 4
    assert np.all(np.diff(lam) >= 0) and np.abs(Q.T @ Q - np.eye(4)).max() <= 1e-12


def test_c_abi_reports_the_loop_and_runs_the_block_cycle():
    """through the C ABI on device-layer handles: kconv, psp_last_solve_info and the block cycle's level vectors"""
    from pysparse_amd import _capi, device as dev
    L = _capi.lib()
    grid = (33, 31)
    n, k = grid[0] * grid[1], 4
    D = dev.DeviceCSR.poisson(*grid)
    K = dev.DeviceMultigrid(D, grid)
    assert K.block_info()["columns"] == 0
    opA, opK = C.c_void_p(), C.c_void_p()
    assert L.psp_op_from_csr(D._h, C.byref(opA)) == 0 and L.psp_op_from_mg(K._h, C.byref(opK)) == 0
    try:
        lam, res, X = np.zeros(k), np.zeros(k), np.full((k, n + 3), np.nan)
        kconv, it = C.c_int(-1), C.c_int(-1)
        rc = L.psp_lobpcg(opA, None, opK, n, k, TOL, 70, None, 0, 0, lam.ctypes.data, X.ctypes.data, n + 3,
                          res.ctypes.data, C.byref(kconv), C.byref(it))
        assert rc == 0, L.psp_last_error()
        assert kconv.value == k and 0 < it.value <= 70
        assert np.abs(lam - poisson_spectrum(grid, k)).max() <= 2 * TOL
        assert np.all(np.isnan(X[:, n:])) and np.all(np.isfinite(X[:, :n]))
        name, info = C.create_string_buffer(64), (C.c_int * 4)()
        assert L.psp_last_solve_info(name, 64, info) == 0
        assert name.value == b"lobpcg" and info[2] == 0  # no restart
        assert K.block_info()["columns"] >= 1  # K was applied as a block, not column by column
        # refusals that need no device come back as PSP_EINVAL
        for kk, nn in ((0, n), (33, n), (4, 11)):
            assert L.psp_lobpcg(opA, None, opK, nn, kk, TOL, 70, None, 0, 0, lam.ctypes.data, X.ctypes.data, n + 3,
                                res.ctypes.data, C.byref(kconv), C.byref(it)) == -1
    finally:
        L.psp_op_destroy(opA)
        L.psp_op_destroy(opK)
