"""CPU: precon.multigrid(..., galerkin=True) / device.DeviceMultigrid(..., galerkin=True) -- the new argument and its
checks before any device call, the new C symbols, and the oracle of the Galerkin V-cycle: the level
operators A_{l+1} = R A_l P from SciPy products, the cycle in float64, and the same cycle in np.longdouble (level operators
from COO triples summed with np.add.reduceat) as the yardstick of both.  tests/test_gpu_multigrid_galerkin.py imports the
oracle and the operator generator from here.  Nothing here needs a GPU.

The tests under "the feature" exercise the library and fail without it.  The tests under "oracle guards" (level lists,
stencil width, symmetry, definiteness, iteration counts, the two legs against each other) guard the yardstick, not the
code: they pass whatever the library does, and are here so that a mistake in the oracle cannot pass for one in the
kernels."""
import functools
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _p1, level_grids, numpy_pcg

LD = np.longdouble
KINDS = ("const", "smooth", "rand100", "rand1e4", "inclusion1e4")

# ------------------------------------------------------------------------------------------------ the test operators


def kappa_field(grid, kind, seed=0):
    """the cell field, shape grid[::-1] (axis 0 of the grid is the fastest index)"""
    shape = tuple(int(g) for g in grid)[::-1]
    rng = np.random.default_rng([seed, len(grid)] + list(grid))
    if kind == "const":
        return np.ones(shape)
    if kind == "smooth":  # exp(sum of sines): max / min = e^6, about 400
        t = np.zeros(shape)
        for ax, m in enumerate(shape):
            x = (np.arange(m) + 0.5) / m
            sh = [1] * len(shape)
            sh[ax] = m
            t = t + np.sin(2.0 * np.pi * x + rng.uniform(0.0, 2.0 * np.pi)).reshape(sh)
        return np.exp(3.0 / len(shape) * t)
    if kind == "rand100":
        return 10.0 ** rng.uniform(0.0, 2.0, shape)
    if kind == "rand1e4":
        return 10.0 ** rng.uniform(0.0, 4.0, shape)
    if kind == "inclusion1e4":  # a box of 10^4 in the middle third of every axis
        k = np.ones(shape)
        k[tuple(slice(m // 3, max(m // 3 + 1, 2 * m // 3)) for m in shape)] = 1.0e4
        return k
    raise ValueError(kind)


def varying_operator(grid, kind, s=0.0, seed=0):
    """-div(kappa grad u) + s u on the grid, cell-centred: the coupling of two neighbours is minus the harmonic mean of
    their kappa, a missing neighbour (Dirichlet end) counts with the cell's own kappa on the diagonal; row
    k = i0 + n0 i1 + n0 n1 i2.  kind 'const' is the project's Poisson operator + s I.  Exactly symmetric."""
    grid = tuple(int(g) for g in grid)
    nd, n = len(grid), int(np.prod(grid))
    kap = kappa_field(grid, kind, seed)
    idx = np.arange(n).reshape(kap.shape)
    diag = np.full(kap.shape, float(s))
    rows, cols, vals = [], [], []
    for a, m in enumerate(grid):
        ax = nd - 1 - a
        if m == 1:
            continue
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[ax], hi[ax] = slice(0, m - 1), slice(1, m)
        lo, hi = tuple(lo), tuple(hi)
        h = 2.0 * kap[lo] * kap[hi] / (kap[lo] + kap[hi])
        low = kap.copy()   # what each point adds for its lower / upper neighbour along the axis
        up = kap.copy()
        low[hi] = h
        up[lo] = h
        diag = diag + low + up
        rows += [idx[lo].ravel(), idx[hi].ravel()]
        cols += [idx[hi].ravel(), idx[lo].ravel()]
        vals += [-h.ravel(), -h.ravel()]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


# ------------------------------------------------------------------------------------------------ the oracle

def _coo_sorted(M):
    """(rows, cols, vals as longdouble, starts of the rows that have entries, those rows) of a SciPy matrix, row-major"""
    C = M.tocoo()
    order = np.lexsort((C.col, C.row))
    return C.row[order], C.col[order], C.data[order].astype(LD)


class _LdMat:
    """a sparse matrix in np.longdouble: sorted COO triples; the product sums each row's terms with np.add.reduceat"""

    def __init__(self, rows, cols, vals, shape):
        self.rows, self.cols, self.vals, self.shape = rows, cols, vals, shape
        self.urows, self.starts = np.unique(rows, return_index=True)

    @classmethod
    def from_scipy(cls, M):
        return cls(*_coo_sorted(M), M.shape)

    def dot(self, x):
        y = np.zeros(self.shape[0], dtype=LD)
        if self.vals.size:
            y[self.urows] = np.add.reduceat(self.vals * x[self.cols], self.starts)
        return y

    def toarray(self):
        D = np.zeros(self.shape, dtype=LD)
        np.add.at(D, (self.rows, self.cols), self.vals)
        return D


def _ld_triple(A, P, scale):
    """P' A P * scale in longdouble: every product P[i, K] A[i, j] P[j, J] as a COO triple, then one sum per (K, J)"""
    Pc = P.tocsr()
    Pc.sort_indices()
    ptr, pj, pv = Pc.indptr, Pc.indices, Pc.data.astype(LD)

    def expand(keep, along, vals):
        """replace the index `along` of every triple by the entries of P's row `along`"""
        cnt = ptr[along + 1] - ptr[along]
        rep = np.repeat(np.arange(along.size), cnt)
        pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(ptr[along], cnt)
        return keep[rep], pj[pos], vals[rep] * pv[pos]

    i, J, v = expand(A.rows, A.cols, A.vals)      # (i, J): A P
    J2, K, v = expand(J, i, v)                     # (J, K): P' A P
    v = v * LD(scale)
    nc = P.shape[1]
    key = K.astype(np.int64) * nc + J2
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    ukey, starts = np.unique(key, return_index=True)
    return _LdMat(ukey // nc, ukey % nc, np.add.reduceat(v, starts), (nc, nc))


class GalerkinOracle:
    """the levels of one operator: A_0 = A, A_{l+1} = R_l A_l P_l with section 9c's P_l and R_l = P_l' / 2^(coarsened
    axes), the smoother weights omega / diag(A_l), and the dense inverse of the coarsest level -- in float64 from SciPy
    (apply) and in np.longdouble (apply_ext)"""

    def __init__(self, grid, A):
        assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended format here: the yardstick is missing"
        self.grids = level_grids(grid)
        self.A, self.P, self.R = [A.tocsr()], [], []
        self.Ax, self.Px, self.Rx = [_LdMat.from_scipy(A)], [], []
        for g in self.grids[:-1]:
            co = [m >= 4 for m in g]
            P = _kron_axes([_p1(m) if k else sp.identity(m, format="csr") for m, k in zip(g, co)]).tocsr()
            scale = 1.0 / 2.0 ** sum(co)
            R = (P.T * scale).tocsr()
            self.P.append(P)
            self.R.append(R)
            Ac = (R @ self.A[-1] @ P).tocsr()
            Ac.sort_indices()
            self.A.append(Ac)
            self.Px.append(_LdMat.from_scipy(P))
            self.Rx.append(_LdMat.from_scipy(R))
            self.Ax.append(_ld_triple(self.Ax[-1], P, scale))
        self.d = [M.diagonal() for M in self.A]
        self.dx = [np.diag(M.toarray()).copy() if M.shape[0] <= 27 else None for M in self.Ax]
        for l, M in enumerate(self.Ax):
            if self.dx[l] is None:
                m = M.rows == M.cols
                d = np.zeros(M.shape[0], dtype=LD)
                d[M.rows[m]] = M.vals[m]
                self.dx[l] = d
        self.inv = np.linalg.inv(self.A[-1].toarray())
        Ad = self.Ax[-1].toarray()
        X = self.inv.astype(LD)
        two = 2.0 * np.eye(Ad.shape[0], dtype=LD)
        for _ in range(2):  # Newton: X <- X (2 I - A X)
            X = X @ (two - Ad @ X)
        self.invx = X

    def apply(self, b, omega=0.8, steps=2, level=0):
        if level == len(self.grids) - 1:
            return self.inv @ b
        A, w = self.A[level], omega / self.d[level]
        x = np.zeros_like(b)
        for _ in range(steps):
            x = x + w * (b - A @ x)
        x = x + self.P[level] @ self.apply(self.R[level] @ (b - A @ x), omega, steps, level + 1)
        for _ in range(steps):
            x = x + w * (b - A @ x)
        return x

    def apply_ext(self, b, omega=0.8, steps=2, level=0):
        b = np.asarray(b, dtype=LD)
        if level == len(self.grids) - 1:
            return self.invx @ b
        A, w = self.Ax[level], LD(omega) / self.dx[level]
        x = np.zeros_like(b)
        for _ in range(steps):
            x = x + w * (b - A.dot(x))
        x = x + self.Px[level].dot(self.apply_ext(self.Rx[level].dot(b - A.dot(x)), omega, steps, level + 1))
        for _ in range(steps):
            x = x + w * (b - A.dot(x))
        return x


@functools.lru_cache(maxsize=None)
def galerkin_oracle_for(grid, kind, s=0.0, seed=0):
    grid = tuple(grid)
    return GalerkinOracle(grid, varying_operator(grid, kind, s, seed))


# ------------------------------------------------------------------------------------------------ the feature

def ll(n, m=None):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, m or n)
    for i in range(min(n, m or n)):
        A[i, i] = 2.0
    return A


class Duck:
    shape = (6, 6)

    def matvec(self, x, y):
        y[:] = x


def test_precon_multigrid_takes_the_keyword():
    from pysparse.precon import precon
    assert "galerkin=False" in precon.multigrid.__doc__
    # a real bool passes the argument parser: what is raised is the ValueError of a later check, not a TypeError
    for flag in (True, False):
        with pytest.raises(ValueError):
            precon.multigrid(ll(6), (7,), galerkin=flag)
        with pytest.raises(ValueError):
            precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2, galerkin=flag)
    with pytest.raises(TypeError):  # a keyword, not a fifth positional argument
        precon.multigrid(ll(6), (7,), 0.8, 2, True)


def test_device_multigrid_has_the_parameter():
    from pysparse_amd import device
    p = inspect.signature(device.DeviceMultigrid.__init__).parameters
    assert list(p)[1:] == ["A", "grid", "omega", "steps", "galerkin"] and p["galerkin"].default is False
    assert hasattr(device.DeviceMultigrid, "level_operator")


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, np.True_, [True]])
def test_a_galerkin_that_is_no_bool_is_a_type_error(bad):
    from pysparse.precon import precon
    from pysparse_amd import device

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing below may reach the library
            self._h = None
            self.shape = shape

    with pytest.raises(TypeError, match="bool"):
        precon.multigrid(ll(6), (6,), galerkin=bad)
    with pytest.raises(TypeError, match="bool"):
        device.DeviceMultigrid(FakeCSR((6, 6)), (6,), galerkin=bad)


def test_precon_multigrid_type_errors_with_galerkin():
    from pysparse.precon import precon
    with pytest.raises(TypeError):
        precon.multigrid(Duck(), (6,), galerkin=True)
    with pytest.raises(TypeError):
        precon.multigrid(ll(6), 6, galerkin=True)
    with pytest.raises(TypeError):
        precon.multigrid(ll(6), galerkin=True)


@pytest.mark.parametrize("n,m,args", [
    (6, 6, ((),)),                 # len(grid) outside 1 .. 3
    (6, 6, ((1, 1, 2, 3),)),
    (6, 6, ((0, 6),)),             # a zero or negative axis
    (6, 6, ((-2, -3),)),
    (6, 6, ((2, 2),)),             # prod(grid) != n
    (6, 6, ((7,),)),
    (6, 5, ((6,),)),               # a rectangular matrix
    (5, 6, ((5,),)),
    (6, 6, ((6,), 0.0)),           # omega <= 0 or > 1
    (6, 6, ((6,), -0.5)),
    (6, 6, ((6,), 1.0000001)),
    (6, 6, ((6,), 0.8, 0)),        # steps < 1
    (6, 6, ((2, 3), 0.8, -1)),
])
def test_precon_multigrid_value_errors_before_any_device_call_with_galerkin(n, m, args):
    """(there is no device here: a call that reached the library would raise RuntimeError, not ValueError)"""
    from pysparse.precon import precon
    with pytest.raises(ValueError):
        precon.multigrid(ll(n, m), *args, galerkin=True)


def test_precon_multigrid_keywords_with_galerkin():
    from pysparse.precon import precon
    with pytest.raises(ValueError):
        precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2, galerkin=True)
    with pytest.raises(ValueError):
        precon.multigrid(ll(6), (6,), steps=0, galerkin=True)


def test_device_layer_refuses_before_any_device_call_with_galerkin():
    from pysparse_amd import device

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing below may reach the library
            self._h = None
            self.shape = shape

    with pytest.raises(TypeError):
        device.DeviceMultigrid(Duck(), (6,), galerkin=True)
    with pytest.raises(TypeError):
        device.DeviceMultigrid(FakeCSR((6, 6)), 6, galerkin=True)
    with pytest.raises(TypeError):
        device.DeviceMultigrid(FakeCSR((6, 6)), (6,), 0.8, 1.9, galerkin=True)  # no silent truncation of steps
    for shape, args in (((6, 6), ((),)), ((6, 6), ((1, 1, 2, 3),)), ((6, 6), ((0, 6),)), ((6, 6), ((2, 2),)),
                        ((6, 5), ((6,),)), ((6, 6), ((6,), 0.0)), ((6, 6), ((6,), 1.5)), ((6, 6), ((6,), 0.8, 0))):
        with pytest.raises(ValueError):
            device.DeviceMultigrid(FakeCSR(shape), *args, galerkin=True)


NEW_SYMBOLS = ("psp_mg_create_csr_galerkin", "psp_mg_create_sss_galerkin", "psp_mg_level_operator", "psp_mg_is_galerkin")


def test_new_symbols_are_declared_and_exported():
    from pysparse_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pysparse_hip.h")) as f:
        header = f.read()
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert getattr(L, name).argtypes is not None, name  # bound with a signature, not only exported


# ------------------------------------------------------------------------------------------------ oracle guards

GUARD_GRIDS = [(7,), (5, 4), (37, 50), (9, 8, 7), (16, 16, 3)]


def test_extended_precision_is_there():
    """fails, not skips: without an extended format the yardstick of the GPU test would be float64 itself"""
    assert np.finfo(LD).eps < 1e-18


def test_operator_generator():
    """'const' is the project's Poisson operator; every kind is exactly symmetric with a positive diagonal, has the axis
    pattern only and is seeded"""
    from test_multigrid_host import grid_operator
    for grid in ((7,), (5, 4), (9, 8, 7), (16, 16, 3)):
        P = grid_operator(grid, (1.0,) * len(grid), 0.3)
        assert abs(varying_operator(grid, "const", 0.3) - P).max() == 0.0
        st = np.cumprod((1,) + grid[:-1])
        for kind in KINDS:
            A = varying_operator(grid, kind, 0.0, 1)
            assert abs(A - A.T).max() == 0.0 and A.diagonal().min() > 0.0
            C = A.tocoo()
            assert set(np.abs(C.col - C.row)) <= set(st) | {0}
            assert abs(A - varying_operator(grid, kind, 0.0, 1)).max() == 0.0
            if kind != "const" and kind != "inclusion1e4":
                assert abs(A - varying_operator(grid, kind, 0.0, 2)).max() > 0.0
    k = kappa_field((37, 50), "smooth")
    assert 100.0 <= k.max() / k.min() <= 404.0
    k = kappa_field((20, 24, 28), "inclusion1e4")
    assert k.max() == 1e4 and k.min() == 1.0 and 0.02 <= (k == 1e4).mean() <= 0.06


@pytest.mark.parametrize("grid", GUARD_GRIDS + [(130, 67), (20, 24, 28)])
def test_level_lists_and_stencil_width(grid):
    O = galerkin_oracle_for(grid, "rand100")
    assert O.grids == level_grids(grid)
    nd = len(grid)
    for l, (g, A) in enumerate(zip(O.grids, O.A)):
        assert A.shape[0] == int(np.prod(g))
        assert np.diff(A.indptr).max() <= 3 ** nd
        # the pattern is the box {-1, 0, 1}^nd of the level's own grid: no entry leaves it
        C = A.tocoo()
        k, j = C.row, C.col
        for m in g:
            assert np.abs(k % m - j % m).max() <= 1
            k, j = k // m, j // m
        # the two legs hold the same operator
        X = O.Ax[l]
        Ad = sp.csr_matrix((X.vals.astype(np.float64), (X.rows, X.cols)), shape=X.shape)
        assert abs(Ad - A).max() <= 1e-13 * abs(A).max()
        assert abs(A - A.T).max() <= 1e-13 * abs(A).max()


@pytest.mark.parametrize("grid", GUARD_GRIDS)
@pytest.mark.parametrize("kind", ["const", "smooth", "rand1e4"])
def test_oracle_cycle_is_symmetric_positive_definite(grid, kind):
    O = galerkin_oracle_for(grid, kind, 0.0)
    n = int(np.prod(grid))
    rng = np.random.default_rng(n)
    for omega, steps in ((0.8, 2), (1.0, 1), (2.0 / 3.0, 3)):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = O.apply(u, omega, steps), O.apply(v, omega, steps)
        assert abs(u @ Mv - v @ Mu) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(Mv)
        assert u @ Mu > 0.0 and v @ Mv > 0.0


@pytest.mark.parametrize("grid", GUARD_GRIDS)
def test_the_two_legs_agree(grid):
    """the float64 leg lies within a few eps of the extended one (what the GPU test's bound is measured in)"""
    eps = np.finfo(np.float64).eps
    for kind, s in (("smooth", 0.0), ("rand1e4", 0.3)):
        O = galerkin_oracle_for(grid, kind, s)
        b = np.random.default_rng(3).standard_normal(int(np.prod(grid)))
        z, zx = O.apply(b), O.apply_ext(b)
        assert zx.dtype == LD
        assert np.abs(z - zx).max() <= 64 * eps * np.abs(zx).max()


@pytest.mark.parametrize("grid", [(37, 50), (130, 67), (20, 24, 28), (33, 31, 35)])
def test_oracle_preconditioned_pcg_counts(grid):
    """the reason for the feature: on varying coefficients Jacobi-PCG needs O(n_axis) iterations, the Galerkin V-cycle
    stays below 20 whatever the grid"""
    counts = {}
    for kind in ("smooth", "rand100", "inclusion1e4"):
        O = galerkin_oracle_for(grid, kind, 0.0)
        A = O.A[0]
        b = np.random.default_rng(1).standard_normal(A.shape[0])
        x, it = numpy_pcg(A, b, 1e-8, 2000, O.apply)
        assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
        dinv = 1.0 / A.diagonal()
        _, itj = numpy_pcg(A, b, 1e-8, 5000, lambda r: dinv * r)
        counts[kind] = (it, itj)
        print(grid, kind, "V-cycle PCG", it, "Jacobi PCG", itj)
        assert it <= 20 and itj >= 4 * it, counts
