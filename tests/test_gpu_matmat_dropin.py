"""GPU: matmat and pcg_batch of the drop-in extension modules (pysparse.sparse.spmatrix, pysparse.itsolvers.krylov):
csr_mat / sss_mat / ll_mat .matmat with C-ordered, Fortran-ordered and sliced (n, k) arrays against matvec per column,
krylov.pcg_batch against krylov.pcg per column with precon.jacobi -- array_equal throughout -- and the errors for wrong
shapes, a wrong dtype and a read-only result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_spmatrix_host import poisson2d, poisson2d_sym  # noqa: E402

NX = 23
K = 5


def blocks(n, k, seed):
    """the same values as a C-ordered, a Fortran-ordered and a sliced array (rows and columns of a larger one)"""
    V = np.random.default_rng(seed).standard_normal((n, k))
    big = np.full((2 * n + 1, 2 * k), np.nan)
    big[1:2 * n + 1:2, ::2] = V
    return {"C": np.ascontiguousarray(V), "F": np.asfortranarray(V), "sliced": big[1:2 * n + 1:2, ::2]}


def results(n, k):
    big = np.full((n + 3, 3 * k), np.nan, order="F")
    return {"C": np.full((n, k), np.nan), "F": np.full((n, k), np.nan, order="F"), "sliced": big[2:n + 2, 1::3]}, big


def per_column(A, X, nrows):
    ref = np.empty((nrows, X.shape[1]))
    for c in range(X.shape[1]):
        y = np.empty(nrows)
        A.matvec(np.ascontiguousarray(X[:, c]), y)
        ref[:, c] = y
    return ref


@pytest.mark.parametrize("kind", ["ll_mat", "ll_mat_sym", "csr_mat", "sss_mat"])
def test_matmat_equals_matvec_per_column(kind):
    L = poisson2d_sym(NX) if kind in ("ll_mat_sym", "sss_mat") else poisson2d(NX)
    A = {"ll_mat": lambda: L, "ll_mat_sym": lambda: L, "csr_mat": L.to_csr, "sss_mat": L.to_sss}[kind]()
    n = NX * NX
    xs = blocks(n, K, 3)
    ref = per_column(A, xs["C"], n)
    for xo, X in xs.items():
        ys, big = results(n, K)
        for yo, Y in ys.items():
            A.matmat(X, Y)
            assert np.array_equal(Y, ref), (kind, xo, yo)
        assert np.isnan(big[:2]).all() and np.isnan(big[n + 2:]).all() and np.isnan(big[:, 0::3]).all()
        assert np.isnan(big[:, 2::3]).all()
    # one column
    Y1 = np.empty((n, 1))
    A.matmat(xs["C"][:, :1], Y1)
    assert np.array_equal(Y1[:, 0], ref[:, 0])


def test_matmat_rectangular_ll_mat():
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(7, 11)
    rng = np.random.default_rng(4)
    for i in range(7):
        for j in rng.choice(11, size=4, replace=False):
            A[i, int(j)] = float(rng.standard_normal())
    X = rng.standard_normal((11, 3))
    Y = np.empty((7, 3))
    A.matmat(X, Y)
    assert np.array_equal(Y, per_column(A, X, 7))
    C = A.to_csr()
    Y2 = np.empty((7, 3), order="F")
    C.matmat(np.asfortranarray(X), Y2)
    assert np.array_equal(Y2, Y)


@pytest.mark.parametrize("kind", ["csr_mat", "sss_mat", "ll_mat"])
def test_matmat_refuses(kind):
    L = poisson2d_sym(6) if kind == "sss_mat" else poisson2d(6)
    A = {"ll_mat": lambda: L, "csr_mat": L.to_csr, "sss_mat": L.to_sss}[kind]()
    n = 36
    with pytest.raises(ValueError):
        A.matmat(np.ones((n + 1, 2)), np.zeros((n, 2)))
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2)), np.zeros((n, 3)))
    with pytest.raises(ValueError):
        A.matmat(np.ones(n), np.zeros(n))
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2), dtype=np.float32), np.zeros((n, 2)))
    with pytest.raises(TypeError):
        A.matmat([[1.0, 1.0]] * n, np.zeros((n, 2)))
    Y = np.zeros((n, 2))
    Y.flags.writeable = False
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2)), Y)


@pytest.mark.parametrize("kind", ["csr_mat", "sss_mat", "ll_mat"])
def test_pcg_batch_equals_pcg_per_column(kind):
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    L = poisson2d_sym(40) if kind == "sss_mat" else poisson2d(40)
    A = {"ll_mat": lambda: L, "csr_mat": L.to_csr, "sss_mat": L.to_sss}[kind]()
    n = 1600
    Kp = precon.jacobi(A, 1.0, 1)
    rng = np.random.default_rng(8)
    B = rng.standard_normal((n, 4))
    B[:, 2] = 0.0
    X0 = np.zeros((n, 4))
    X0[:, 1] = rng.standard_normal(n)
    X0[:, 2] = 1.0
    for name, X in blocks(n, 4, 0).items():
        X[...] = X0
        info, it, rr = krylov.pcg_batch(A, np.asfortranarray(B) if name == "F" else B, X, 1e-9, 500, Kp)
        assert info.shape == it.shape == rr.shape == (4,)
        for c in range(4):
            x = np.ascontiguousarray(X0[:, c])
            i1, t1, r1 = krylov.pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-9, 500, Kp)
            assert (int(info[c]), int(it[c])) == (i1, t1) and float(rr[c]) == r1, (kind, name, c)
            assert np.array_equal(X[:, c], x), (kind, name, c)
        assert info[2] == 0 and it[2] == 0 and not X[:, 2].any()
    # without a preconditioner
    X = X0.copy()
    info, it, rr = krylov.pcg_batch(A, B, X, 1e-9, 500)
    x = np.ascontiguousarray(X0[:, 0])
    assert krylov.pcg(A, np.ascontiguousarray(B[:, 0]), x, 1e-9, 500) == (int(info[0]), int(it[0]), float(rr[0]))
    assert np.array_equal(X[:, 0], x)


def test_pcg_batch_refuses():
    from pysparse.itsolvers import krylov
    A = poisson2d(6).to_csr()
    n = 36
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((n, 2)), np.zeros((n, 3)), 1e-8, 10)
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((n + 1, 2)), np.zeros((n + 1, 2)), 1e-8, 10)
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones(n), np.zeros(n), 1e-8, 10)
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((n, 2), dtype=np.float32), np.zeros((n, 2)), 1e-8, 10)
    with pytest.raises(TypeError):
        krylov.pcg_batch(A, [[1.0, 1.0]] * n, np.zeros((n, 2)), 1e-8, 10)
    X = np.zeros((n, 2))
    X.flags.writeable = False
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((n, 2)), X, 1e-8, 10)
    # a matrix on a device list (one GPU listed twice), where the runtime lets one be built
    try:
        AM = poisson2d(6).to_csr(devices=[0, 0])
    except Exception:  # noqa: BLE001 - no second rank on this runtime: nothing to refuse
        AM = None
    if AM is not None:
        with pytest.raises(ValueError):
            krylov.pcg_batch(AM, np.ones((n, 2)), np.zeros((n, 2)), 1e-8, 10)
        with pytest.raises(ValueError):
            AM.matmat(np.ones((n, 2)), np.zeros((n, 2)))
