"""GPU: psp_pcg_batch -- k PCG recurrences advanced by one loop -- against psp_pcg run alone on each column of the same
handle: info and iter ==, relres equal as floats, x array_equal.  No tolerance anywhere: the batched kernels form and add
their partial sums in the single solve's order.

Columns of B (in this order, a case with k columns takes the first k): A.1, a random column, a zero column (x := 0,
info 0, iter 0), a column whose x0 already is the solution (info 0, iter 0), a smooth column that converges in a few
iterations -- so it stays frozen beside rough ones for many iterations -- and random columns.  Every column's block
column of X must equal the single solve's x, which is also what shows that a frozen column is not written again while
the loop goes on for the others.

The breakdown column (info -6) is the indefinite diagonal operator of test_stagnation_and_breakdown_codes (p.Ap == 0 in
the first iteration) beside a column supported on its positive half, which converges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
KMAX = 9


def smooth_column(nx, ny):
    i = np.arange(1, nx + 1)
    j = np.arange(1, ny + 1)
    return np.outer(np.sin(np.pi * j / (ny + 1)), np.sin(np.pi * i / (nx + 1))).ravel()  # an eigenvector of the 5-point operator


def irregular_spd(n, seed):
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    r = np.repeat(np.arange(n), 4)
    c = rng.integers(0, n, size=r.size)
    M[r, c] = -rng.uniform(0.1, 1.0, size=r.size)
    M = np.triu(M, 1)
    M = M + M.T
    # strongly dominant: a few dozen iterations per solve, so that all the single solves of this file together stay far
    # below the 2048 products after which the handle would move to its renumbered copy
    M[np.arange(n), np.arange(n)] = 2.0 * np.abs(M).sum(axis=1) + rng.uniform(0.5, 1.0, size=n)
    return M


def csr_arrays(M):
    r, c = np.nonzero(M)
    ind = np.zeros(M.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=M.shape[0]), out=ind[1:])
    return ind, c.astype(np.int32), np.ascontiguousarray(M[r, c])


class System:
    """a handle, its B / X0 blocks (n x ncols) and the single solves, each computed once"""

    def __init__(self, A, n, smooth=None, seed=0, ncols=KMAX):
        self.A, self.n = A, n
        rng = np.random.default_rng(seed)
        B = rng.standard_normal((n, ncols))
        X0 = np.zeros((n, ncols))
        y = np.empty(n)
        A.matvec(np.ones(n), y)
        B[:, 0] = y
        if ncols > 2:
            B[:, 2] = 0.0
            X0[:, 2] = rng.standard_normal(n)  # must come back as zeros
        if ncols > 3:
            X0[:, 3] = rng.standard_normal(n)
            A.matvec(np.ascontiguousarray(X0[:, 3]), y)
            B[:, 3] = y
        if smooth is not None and ncols > 4:
            B[:, 4] = smooth
        if ncols > 6:
            X0[:, 6] = rng.standard_normal(n)  # a nonzero initial guess
        self.B, self.X0 = B, X0
        self.single = {}

    def solve_alone(self, c, maxit, K, kname):
        from pysparse_amd.device import pcg
        key = (c, maxit, kname)
        if key not in self.single:
            x = np.ascontiguousarray(self.X0[:, c])
            res = pcg(self.A, np.ascontiguousarray(self.B[:, c]), x, TOL, maxit, K)
            self.single[key] = (res, x)
        return self.single[key]


_systems = {}


def system(name):
    from pysparse_amd.device import DeviceCSR, DeviceSSS
    if name not in _systems:
        if name == "csr33x31":
            _systems[name] = System(DeviceCSR.poisson(33, 31), 33 * 31, smooth_column(33, 31), 1)
        elif name == "sss33x31":
            _systems[name] = System(DeviceSSS.poisson(33, 31), 33 * 31, smooth_column(33, 31), 2)
        elif name == "csr100x100":
            _systems[name] = System(DeviceCSR.poisson(100, 100), 10000, smooth_column(100, 100), 3)
        elif name == "sss100x100":
            _systems[name] = System(DeviceSSS.poisson(100, 100), 10000, smooth_column(100, 100), 4)
        elif name == "irregular3000":
            M = irregular_spd(3000, 5)
            ind, col, val = csr_arrays(M)
            A = DeviceCSR.from_arrays(M.shape, ind, col, val)
            assert A.setup_info()["reorder_state"] != 1
            _systems[name] = System(A, 3000, None, 6)
    return _systems[name]


class CallbackJacobi:
    """a Python preconditioner: the library sees a host callback"""

    def __init__(self, n, d):
        self.shape = (n, n)
        self.dinv = 1.0 / d

    def precon(self, x, y):
        y[:] = x * self.dinv


def make_precon(kname, S):
    from pysparse_amd.device import DeviceJacobi, DeviceSSOR, DeviceSSS
    if kname == "none":
        return None
    if kname == "jacobi1":
        return DeviceJacobi(S.A, 1.0, 1)
    if kname == "jacobi2":
        return DeviceJacobi(S.A, 0.8, 2)
    if kname == "ssor":
        assert isinstance(S.A, DeviceSSS)
        return DeviceSSOR(S.A, 1.3, 1)
    if kname == "callback":
        return CallbackJacobi(S.n, 4.0 + np.arange(S.n) % 3)
    raise KeyError(kname)


def check_batch(S, K, kname, k, pad, maxit):
    from pysparse_amd.device import pcg_batch
    n = S.n
    Xbig = np.full((n + pad, k), np.nan, order="F")
    Bbig = np.full((n + pad, k), np.nan, order="F")
    X, B = Xbig[:n], Bbig[:n]
    X[...] = S.X0[:, :k]
    B[...] = S.B[:, :k]
    info, it, rr = pcg_batch(S.A, B, X, TOL, maxit, K)
    assert np.isnan(Xbig[n:]).all()
    for c in range(k):
        (i1, it1, rr1), x1 = S.solve_alone(c, maxit, K, kname)
        print(kname, "k", k, "pad", pad, "maxit", maxit, "col", c, "batch", (info[c], it[c], rr[c]), "alone", (i1, it1, rr1))
        assert info[c] == i1 and it[c] == it1, (c, k, pad)
        assert float(rr[c]) == float(rr1), (c, k, pad)
        assert np.array_equal(X[:, c], x1), (c, k, pad)
    return info, it


CASES = [("csr33x31", "none"), ("csr33x31", "jacobi1"), ("csr33x31", "jacobi2"), ("csr33x31", "callback"),
         ("sss33x31", "none"), ("sss33x31", "jacobi1"), ("sss33x31", "jacobi2"), ("sss33x31", "ssor"),
         ("csr100x100", "none"), ("csr100x100", "jacobi1"), ("csr100x100", "jacobi2"),
         ("sss100x100", "jacobi1"), ("sss100x100", "ssor"),
         ("irregular3000", "none"), ("irregular3000", "jacobi1"), ("irregular3000", "jacobi2")]


@pytest.mark.parametrize("sysname,kname", CASES)
def test_columns_equal_single_solves(sysname, kname):
    S = system(sysname)
    K = make_precon(kname, S)
    slow = kname in ("callback", "jacobi2", "ssor") or sysname.endswith("100x100")
    for k in ((3, 9) if slow else (1, 3, 8, 9)):
        for pad in ((5,) if slow and k == 9 else (0, 5)):
            info, it = check_batch(S, K, kname, k, pad, 2000)
            assert info[0] == 0
            if k > 3:
                assert info[2] == 0 and it[2] == 0 and info[3] == 0 and it[3] == 0
            if k > 5 and sysname != "irregular3000":
                assert it[4] < it[5]  # the smooth column froze long before the rough one
    if sysname == "irregular3000":
        assert S.A.setup_info()["reorder_state"] != 1


@pytest.mark.parametrize("sysname,kname", [("csr33x31", "none"), ("sss33x31", "jacobi1"), ("csr100x100", "jacobi1"),
                                           ("irregular3000", "none")])
def test_some_columns_run_out(sysname, kname):
    S = system(sysname)
    K = make_precon(kname, S)
    maxit = 5
    for k in (8, 9):
        info, it = check_batch(S, K, kname, k, 5, maxit)
        assert info[1] == -1 and it[1] == maxit + 1
        assert info[2] == 0 and info[3] == 0
        if sysname != "irregular3000":
            assert info[4] == 0 and it[4] <= maxit  # the smooth column converged while others ran out


def test_loop_is_named_and_launches_do_not_grow_with_k():
    from pysparse_amd.device import DeviceJacobi, last_solve_info, pcg_batch
    S = system("csr100x100")
    for K in (None, DeviceJacobi(S.A, 1.0, 1)):
        seen = []
        for k in (2, 8):
            X = np.asfortranarray(np.zeros((S.n, k)))
            B = np.asfortranarray(S.B[:, :k] + 1.0)
            pcg_batch(S.A, B, X, TOL, 50, K)
            name, d = last_solve_info()
            assert name == "pcg_batch"
            seen.append(d["launches"])
        assert seen[0] == seen[1] and seen[0] > 0


def test_breakdown_column():
    from pysparse_amd.device import DeviceCSR, pcg, pcg_batch
    n = 64
    ind = np.arange(n + 1, dtype=np.int32)
    col = np.arange(n, dtype=np.int32)
    val = np.ones(n)
    val[n // 2:] = -1.0
    A = DeviceCSR.from_arrays((n, n), ind, col, val)
    B = np.ones((n, 3), order="F")
    B[n // 2:, 1] = 0.0  # lives on the positive half: converges
    B[:, 2] = np.arange(n) % 2  # p.Ap == 0 again
    X = np.zeros((n, 3), order="F")
    info, it, rr = pcg_batch(A, B, X, 1e-10, 50)
    for c in range(3):
        x = np.zeros(n)
        r1 = pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-10, 50)
        assert (info[c], it[c]) == r1[:2] and float(rr[c]) == float(r1[2])
        assert np.array_equal(X[:, c], x)
    assert info[0] == -6 and info[1] == 0 and info[2] == -6


def test_refused_arguments():
    from pysparse_amd._capi import PspError
    from pysparse_amd.device import DeviceCSR, pcg_batch
    S = system("csr33x31")
    n = S.n
    with pytest.raises(ValueError):
        pcg_batch(S.A, np.ones((n, 2)), np.zeros((n, 3)), TOL, 10)
    with pytest.raises(ValueError):
        pcg_batch(S.A, np.ones((n + 1, 2)), np.zeros((n + 1, 2)), TOL, 10)
    with pytest.raises(ValueError):
        pcg_batch(S.A, np.ones((n, 2), dtype=np.float32), np.zeros((n, 2)), TOL, 10)
    with pytest.raises(TypeError):
        pcg_batch(S.A, [[1.0, 1.0]] * n, np.zeros((n, 2)), TOL, 10)
    ro = np.zeros((n, 2))
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        pcg_batch(S.A, np.ones((n, 2)), ro, TOL, 10)
    try:
        AM = DeviceCSR.poisson_multi(33, 31, devices=[0, 0])
    except PspError:
        AM = None
    if AM is not None:
        with pytest.raises(ValueError):
            pcg_batch(AM, np.ones((n, 2)), np.zeros((n, 2)), TOL, 10)
