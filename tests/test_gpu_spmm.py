"""GPU: block products Y[:, c] = A X[:, c] (psp_csr_matmat / psp_sss_matmat and their _dev forms) against the
single-vector products of the SAME handle, column by column, bit for bit.

Every comparison is np.array_equal with psp_csr_matvec / psp_sss_matvec: all kernels add a row's separately rounded
products left to right, so no tolerance is needed.  For each matrix: k in {1, 2, 3, 7, 8, 9, 17}, leading dimensions
n, n + 5, n + 6 (even and odd, so both alignments of a column start), padding rows and a (k+1)-th column pre-filled with
NaN that must still be NaN afterwards, and two runs with equal bits.

Which handles multiply index-free: ensure_w4 refuses layouts whose padded value blocks (whole blocks of 128 rows) would
move more bytes than the CSR arrays (8 * slots > 11 * nnz), so of the grids below the plain DeviceCSR.poisson handle is
csr_spmv_w4 for 16x8, 23x23, 32x16 and 27x19 only -- that expectation is worked out from the rule, see W4_PLAIN -- and
the others go through the general kernel.  DeviceCSR.poisson_big builds the index-free layout directly, whatever the
size (from 2 x 2 on), so every grid but 1x2 is ALSO run through such a handle, where psp_csr_kernel_info must name
csr_spmv_w4."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 7, 8, 9, 17)
KMAX = max(KS)
GRIDS = [(1, 2, 0), (7, 9, 0), (16, 8, 0), (43, 3, 0), (23, 23, 0), (32, 16, 0), (27, 19, 0), (5, 6, 7)]
W4_PLAIN = {(16, 8, 0), (23, 23, 0), (32, 16, 0), (27, 19, 0)}  # 8 * ceil(n / 128) * 128 * offsets <= 11 * nnz


def _lib():
    from pysparse_amd._capi import lib
    return lib()


def _cols(ncols, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((ncols, KMAX)))


def _reference(A, X, nrows):
    """matvec of the same handle, once per column"""
    ref = np.empty((nrows, X.shape[1]), order="F")
    for c in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, c])
        y = np.empty(nrows)
        A.matvec(x, y)
        ref[:, c] = y
    return ref


def _run_dev(A, X, k, ldx, ldy, nrows, ncols):
    """one _dev call on NaN-padded blocks; returns the whole Y block (ldy, k + 1)"""
    from pysparse_amd.device import DeviceBuffer
    Xb = np.full((ldx, k + 1), np.nan, order="F")
    Xb[:ncols, :k] = X[:, :k]
    Yb = np.full((ldy, k + 1), np.nan, order="F")
    dx = DeviceBuffer.from_host(Xb.ravel(order="F"))
    dy = DeviceBuffer.from_host(Yb.ravel(order="F"))
    A.matmat_dev(k, dx.ptr, ldx, dy.ptr, ldy)
    _lib().psp_synchronize()
    out = dy.download().reshape((ldy, k + 1), order="F")
    assert np.array_equal(dx.download().reshape((ldx, k + 1), order="F"), Xb, equal_nan=True)  # X is only read
    dx.free()
    dy.free()
    return out


def check_handle(A, nrows, ncols, seed=0):
    X = _cols(ncols, seed)
    ref = _reference(A, X, nrows)
    for k in KS:
        for pad in (0, 5, 6):
            ldx, ldy = ncols + pad, nrows + pad
            out = _run_dev(A, X, k, ldx, ldy, nrows, ncols)
            assert np.array_equal(out[:nrows, :k], ref[:, :k]), (k, pad)
            assert np.isnan(out[nrows:, :]).all() and np.isnan(out[:, k]).all(), (k, pad)
            if pad == 5:
                again = _run_dev(A, X, k, ldx, ldy, nrows, ncols)
                assert np.array_equal(out, again, equal_nan=True), (k, pad)
        # host blocks: C order, Fortran order with padding rows, and a strided slice
        Yc = np.full((nrows, k), np.nan)
        A.matmat(np.ascontiguousarray(X[:, :k]), Yc)
        assert np.array_equal(Yc, ref[:, :k]), k
    big = np.full((nrows + 3, 2 * KMAX), np.nan, order="F")
    Yv = big[:nrows, ::2]
    A.matmat(X, Yv)
    assert np.array_equal(Yv, ref)
    assert np.isnan(big[nrows:, :]).all() and np.isnan(big[:, 1::2]).all()


def csr_from_dense(M):
    r, c = np.nonzero(M)
    ind = np.zeros(M.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=M.shape[0]), out=ind[1:])
    return ind, c.astype(np.int32), np.ascontiguousarray(M[r, c])


def device_csr(M):
    from pysparse_amd.device import DeviceCSR
    ind, col, val = csr_from_dense(M)
    return DeviceCSR.from_arrays(M.shape, ind, col, val)


def device_sss(M):
    from pysparse_amd.device import DeviceSSS
    L = np.tril(M, -1)
    ind, col, val = csr_from_dense(L)
    return DeviceSSS.from_arrays(M.shape[0], ind, col, val, np.ascontiguousarray(np.diag(M)))


def nine_point(nx, ny):
    n = nx * ny
    M = np.zeros((n, n))
    rng = np.random.default_rng(5)
    for j in range(ny):
        for i in range(nx):
            r = j * nx + i
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    if 0 <= i + di < nx and 0 <= j + dj < ny:
                        M[r, (j + dj) * nx + i + di] = 8.0 if (di == 0 and dj == 0) else -rng.uniform(0.5, 1.5)
    return M


def random_rect(m, n, seed, max_row=9, empty_frac=0.1, long_rows=()):
    rng = np.random.default_rng(seed)
    M = np.zeros((m, n))
    for i in range(m):
        L = 0 if rng.random() < empty_frac else int(rng.integers(0, max_row + 1))
        for r, ln in long_rows:
            if r == i:
                L = ln
        cols = rng.choice(n, size=min(L, n), replace=False)
        M[i, cols] = rng.standard_normal(cols.size) + 3.0  # never exactly zero
    return M


def symmetric(M):
    U = np.triu(M, 1)
    return U + U.T + np.diag(np.diag(M))


def banded(n, half, per_row, seed):
    """random entries inside a band of 2 * half + 1, far more distinct offsets than the index-free layouts take"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    for i in range(n):
        lo, hi = max(0, i - half), min(n, i + half + 1)
        cols = rng.choice(np.arange(lo, hi), size=min(per_row, hi - lo), replace=False)
        M[i, cols] = rng.standard_normal(cols.size) + 3.0
        M[i, i] = 10.0
    return M


def offsets_matrix(n, offs, seed):
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    for o in offs:
        i = np.arange(max(0, -o), min(n, n - o))
        M[i, i + o] = rng.standard_normal(i.size) + 3.0
    return M


def kernel_name(A):
    return A.kernel_info()[0]


@pytest.mark.parametrize("grid", GRIDS)
def test_index_free_poisson(grid):
    from pysparse_amd.device import DeviceCSR
    nx, ny, nz = grid
    n = nx * ny * (nz if nz else 1)
    A = DeviceCSR.poisson(*grid)
    if grid in W4_PLAIN:
        assert kernel_name(A) == "csr_spmv_w4"
    check_handle(A, n, n, seed=1)
    if min(nx, ny) >= 2:  # psp_csr_poisson_big refuses grids with a dimension below 2
        B = DeviceCSR.poisson_big(*grid)
        assert kernel_name(B) == "csr_spmv_w4"
        check_handle(B, n, n, seed=2)


def test_index_free_nine_point_and_released_arrays():
    M = nine_point(24, 23)
    A = device_csr(M)
    assert kernel_name(A) == "csr_spmv_w4"
    check_handle(A, M.shape[0], M.shape[1], seed=3)
    A.release_arrays()
    assert kernel_name(A) == "csr_spmv_w4"
    check_handle(A, M.shape[0], M.shape[1], seed=4)


GENERAL = {
    "n1": lambda: np.array([[2.5]]),
    "rect300x170": lambda: random_rect(300, 170, 11),
    "n2049_empty_and_long_row": lambda: random_rect(2049, 2049, 12, long_rows=((1030, 1500),)),
    "banded_w3": lambda: banded(3000, 150, 12, 13),
    "offsets24_w4x": lambda: offsets_matrix(2048, list(range(-12, 12)), 14),
    "offsets40_w4y": lambda: offsets_matrix(2048, list(range(-20, 20)), 15),
}


@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_path(name):
    M = GENERAL[name]()
    A = device_csr(M)
    kn, info = A.kernel_info()
    print(name, kn, info)
    if name == "banded_w3":
        assert kn == "csr_spmv_w3"
    if name.startswith("offsets"):
        assert kn == "csr_spmv_w4" and info["nb"] == int(name[7:9])  # 32- / 64-bit masks: no block form, general kernel
    check_handle(A, M.shape[0], M.shape[1], seed=6)


SYMMETRIC = {
    "n1": lambda: np.array([[2.5]]),
    "n2049_empty_and_long_row": lambda: symmetric(random_rect(2049, 2049, 21, long_rows=((3, 1500),))),
    "banded": lambda: symmetric(banded(3000, 150, 12, 22)),
    "offsets40": lambda: symmetric(offsets_matrix(2048, list(range(-20, 21)), 23)),
    "nine_point_w4": lambda: symmetric(nine_point(24, 23)),
}


@pytest.mark.parametrize("name", sorted(SYMMETRIC))
def test_sss_mirror_and_index_free(name):
    M = SYMMETRIC[name]()
    S = device_sss(M)
    kn, info = S.kernel_info()
    print(name, kn, info)
    if name == "nine_point_w4":
        assert kn == "sss_spmv_w4"
    check_handle(S, M.shape[0], M.shape[0], seed=7)


@pytest.mark.parametrize("grid", [(23, 23, 0), (5, 6, 7)])
def test_sss_poisson(grid):
    from pysparse_amd.device import DeviceSSS
    S = DeviceSSS.poisson(*grid)
    n = S.n
    if grid == (23, 23, 0):
        assert S.kernel_info()[0] == "sss_spmv_w4"
    check_handle(S, n, n, seed=8)


def test_refused_arguments():
    from pysparse_amd._capi import PspError
    from pysparse_amd.device import DeviceBuffer, DeviceCSR, DeviceSSS
    L = _lib()
    A = DeviceCSR.poisson(23, 23)
    S = DeviceSSS.poisson(23, 23)
    n = 529
    dx = DeviceBuffer.from_host(np.ones(4 * n))
    dy = DeviceBuffer.from_host(np.zeros(4 * n))
    hx, hy = np.ones((n, 2), order="F"), np.zeros((n, 2), order="F")
    px, py = hx.ctypes.data_as(C.c_void_p), hy.ctypes.data_as(C.c_void_p)
    EINVAL = -1
    for fn, h in ((L.psp_csr_matmat_dev, A._h), (L.psp_sss_matmat_dev, S._h)):
        assert fn(h, 2, dx.ptr, n, dx.ptr, n) == EINVAL                  # X and Y the same block
        assert fn(h, 2, dx.ptr, n, dx.ptr + 8 * (2 * n - 1), n) == EINVAL  # overlapping by one element
        assert fn(h, 0, dx.ptr, n, dy.ptr, n) == EINVAL
        assert fn(h, -1, dx.ptr, n, dy.ptr, n) == EINVAL
        assert fn(h, 2, dx.ptr, n - 1, dy.ptr, n) == EINVAL
        assert fn(h, 2, dx.ptr, n, dy.ptr, n - 1) == EINVAL
        assert fn(h, 2, dx.ptr, n, dy.ptr, n) == 0
    for fn, h in ((L.psp_csr_matmat, A._h), (L.psp_sss_matmat, S._h)):
        assert fn(h, 2, px, n, px, n) == EINVAL
        assert fn(h, 0, px, n, py, n) == EINVAL
        assert fn(h, 2, px, n - 1, py, n) == EINVAL
        assert fn(h, 2, px, n, py, n) == 0
    assert L.psp_last_error() is not None
    L.psp_synchronize()
    # Python layer: shapes, dtypes and a read-only result are refused before any device call
    with pytest.raises(ValueError):
        A.matmat(np.ones((n + 1, 2)), np.zeros((n, 2)))
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2)), np.zeros((n, 3)))
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2), dtype=np.float32), np.zeros((n, 2)))
    with pytest.raises(TypeError):
        A.matmat([[1.0] * 2] * n, np.zeros((n, 2)))
    ro = np.zeros((n, 2))
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        A.matmat(np.ones((n, 2)), ro)
    # a two-rank device-list handle (one GPU listed twice), where the runtime lets one be built
    try:
        AM = DeviceCSR.poisson_multi(23, 23, devices=[0, 0])
    except PspError:
        AM = None
    if AM is not None:
        assert L.psp_csr_matmat(AM._h, 2, px, n, py, n) == EINVAL
        assert L.psp_csr_matmat_dev(AM._h, 2, dx.ptr, n, dy.ptr, n) == EINVAL
        assert b"multi-device" in L.psp_last_error()


def test_op_apply_block_every_operator_kind():
    """psp_op_apply_block_dev: csr / sss block kernels, jacobi (steps = 1) one scaling kernel, jacobi (steps = 2), ssor and a
    host callback column by column -- each column with the bits of the operator applied to it alone."""
    from pysparse_amd.device import DeviceBuffer, DeviceCSR, DeviceJacobi, DeviceSSOR, DeviceSSS, _Op
    L = _lib()
    A = DeviceCSR.poisson(27, 19)
    S = DeviceSSS.poisson(27, 19)
    n, k = 513, 5
    X = np.asfortranarray(np.random.default_rng(9).standard_normal((n, k)))

    class Scale:
        shape = (n, n)

        def matvec(self, x, y):
            y[:] = 3.0 * x

    cases = [(A, "matvec", A.matvec), (S, "matvec", S.matvec)]
    for K in (DeviceJacobi(A, 1.0, 1), DeviceJacobi(A, 0.9, 2), DeviceSSOR(S, 1.2, 1)):
        cases.append((K, "precon", K.precon))
    cases.append((Scale(), "matvec", Scale().matvec))
    for obj, method, apply1 in cases:
        op = _Op(obj, method)
        ref = np.empty((n, k), order="F")
        for c in range(k):
            y = np.empty(n)
            apply1(np.ascontiguousarray(X[:, c]), y)
            ref[:, c] = y
        dx = DeviceBuffer.from_host(X.ravel(order="F"))
        dy = DeviceBuffer.from_host(np.full(n * k, np.nan))
        assert L.psp_op_apply_block_dev(op._h, k, dx.ptr, n, dy.ptr, n) == 0, L.psp_last_error()
        L.psp_synchronize()
        out = dy.download().reshape((n, k), order="F")
        assert np.array_equal(out, ref), type(obj).__name__
        op.close()
