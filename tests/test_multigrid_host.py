"""CPU: precon.multigrid / device.DeviceMultigrid -- presence in the alias package, the argument checks that are reached
before any device call, and the SciPy oracle of the V-cycle (the normative definition of DESIGN.md section 9c rebuilt
from Kronecker products), checked against itself.  tests/test_gpu_multigrid.py imports the oracle from here.
Nothing here needs a GPU.

The presence and argument-check tests exercise the feature and fail without it.  The tests of the oracle (level lists,
transfer operators, symmetry, definiteness, iteration counts) guard the yardstick, not the code: they pass whatever the
library does, and are here so that a mistake in the oracle cannot pass for one in the kernels."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

# ------------------------------------------------------------------------------------------------ the oracle


def level_grids(grid):
    """the level grids, finest first: an axis is halved while it has at least 4 points, each axis on its own"""
    out = [tuple(int(g) for g in grid)]
    while any(g >= 4 for g in out[-1]):
        out.append(tuple(g // 2 if g >= 4 else g for g in out[-1]))
    return out


def _t1(n):
    return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


def _kron_axes(mats):
    """(x)_a mats[a] with axis 0 the fastest index: row k = i0 + n0 i1 + n0 n1 i2"""
    out = mats[0]
    for m in mats[1:]:
        out = sp.kron(m, out, format="csr")
    return out


def grid_operator(grid, c, s):
    """A = sum_a c_a T_a + s I; axes of length 1 have no couplings and count as c_a = 0"""
    n = int(np.prod(grid))
    A = s * sp.identity(n, format="csr")
    for a, (g, ca) in enumerate(zip(grid, c)):
        if g > 1:
            A = A + ca * _kron_axes([_t1(m) if b == a else sp.identity(m, format="csr") for b, m in enumerate(grid)])
    return A.tocsr()


def _p1(n):
    """coarse point j sits at fine index 2j + 1; its neighbours 2j and 2j + 2 take one half where they exist"""
    nc = n // 2
    j = np.arange(nc)
    up = j[2 * j + 2 < n]
    rows = np.concatenate([2 * j + 1, 2 * j, 2 * up + 2])
    cols = np.concatenate([j, j, up])
    vals = np.concatenate([np.ones(nc), 0.5 * np.ones(nc), 0.5 * np.ones(up.size)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, nc))


class CycleOracle:
    """the levels of one operator: A_l, P_l, R_l = P_l' / 2^(coarsened axes), d_l = 2 sum_{n_a > 1} c_a + s, and the
    dense inverse of the coarsest level"""

    def __init__(self, grid, c, s):
        self.grids = level_grids(grid)
        self.A, self.P, self.R, self.d = [], [], [], []
        c = [float(x) for x in c]
        for g in self.grids:
            self.A.append(grid_operator(g, c, s))
            self.d.append(2.0 * sum(ca for m, ca in zip(g, c) if m > 1) + s)
            co = [m >= 4 for m in g]
            if any(co):
                P = _kron_axes([_p1(m) if k else sp.identity(m, format="csr") for m, k in zip(g, co)])
                self.P.append(P)
                self.R.append((P.T / 2.0 ** sum(co)).tocsr())
                c = [ca / 4.0 if k else ca for ca, k in zip(c, co)]
        self.inv = np.linalg.inv(self.A[-1].toarray())

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


@functools.lru_cache(maxsize=None)
def oracle_for(grid, c=None, s=0.0):
    grid = tuple(grid)
    return CycleOracle(grid, tuple(c) if c is not None else (1.0,) * len(grid), s)


def numpy_pcg(A, b, tol, maxit, precon):
    """the loop of the library's pcg (zero initial guess, test ||r|| <= tol ||b|| on the recurrence residual); returns
    (x, iterations)"""
    x = np.zeros_like(b)
    r = b.copy()
    tolb = tol * np.linalg.norm(b)
    rho, p = 1.0, None
    for it in range(1, maxit + 1):
        z = precon(r) if precon is not None else r.copy()
        rho1, rho = rho, r @ z
        p = z if it == 1 else z + (rho / rho1) * p
        q = A @ p
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        if np.linalg.norm(r) <= tolb:
            return x, it
    return x, maxit + 1


# ------------------------------------------------------------------------------------------------ the tests

def test_alias_package_exposes_multigrid():
    from pysparse.precon import precon
    import pysparse_amd.precon.precon as p2
    from pysparse_amd import device
    assert callable(precon.multigrid) and precon.multigrid is p2.multigrid
    assert callable(device.DeviceMultigrid)
    for name in ("precon", "precon_dev", "info", "close"):
        assert hasattr(device.DeviceMultigrid, name)


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


def test_precon_multigrid_type_errors():
    from pysparse.precon import precon
    with pytest.raises(TypeError):
        precon.multigrid(Duck(), (6,))
    with pytest.raises(TypeError):
        precon.multigrid(ll(6), 6)
    with pytest.raises(TypeError):
        precon.multigrid(ll(6))


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
def test_precon_multigrid_value_errors_before_any_device_call(n, m, args):
    """(there is no device here: a call that reached the library would raise RuntimeError, not ValueError)"""
    from pysparse.precon import precon
    with pytest.raises(ValueError):
        precon.multigrid(ll(n, m), *args)


def test_precon_multigrid_keywords():
    from pysparse.precon import precon
    with pytest.raises(ValueError):
        precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2)
    with pytest.raises(ValueError):
        precon.multigrid(ll(6), (6,), steps=0)


def test_device_layer_refuses_before_any_device_call():
    from pysparse_amd import device

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing below may reach the library
            self._h = None
            self.shape = shape

    with pytest.raises(TypeError):
        device.DeviceMultigrid(Duck(), (6,))
    with pytest.raises(TypeError):
        device.DeviceMultigrid(FakeCSR((6, 6)), 6)
    with pytest.raises(TypeError):
        device.DeviceMultigrid(FakeCSR((6, 6)), (6,), 0.8, 1.9)  # no silent truncation of steps
    for shape, args in (((6, 6), ((),)), ((6, 6), ((1, 1, 2, 3),)), ((6, 6), ((0, 6),)), ((6, 6), ((2, 2),)),
                        ((6, 5), ((6,),)), ((6, 6), ((6,), 0.0)), ((6, 6), ((6,), 1.5)), ((6, 6), ((6,), 0.8, 0))):
        with pytest.raises(ValueError):
            device.DeviceMultigrid(FakeCSR(shape), *args)


def test_level_lists():
    assert level_grids((130, 67)) == [(130, 67), (65, 33), (32, 16), (16, 8), (8, 4), (4, 2), (2, 2)]
    assert level_grids((64, 64, 3)) == [(64, 64, 3), (32, 32, 3), (16, 16, 3), (8, 8, 3), (4, 4, 3), (2, 2, 3)]
    assert level_grids((3, 3, 3)) == [(3, 3, 3)]
    assert level_grids((7,)) == [(7,), (3,)]
    assert level_grids((5000,))[-1] == (2,) and len(level_grids((5000,))) == 12
    assert level_grids((70, 66, 65))[-1] == (2, 2, 2) and len(level_grids((70, 66, 65))) == 6
    assert level_grids((5, 4)) == [(5, 4), (2, 2)]
    for g in ((37, 50), (9, 8, 7), (20, 24, 28), (33, 31, 35), (48, 48, 48)):
        lv = level_grids(g)
        assert all(m <= 3 for m in lv[-1]) and int(np.prod(lv[-1])) <= 27
        assert oracle_for(g).grids == lv


def test_oracle_operator_is_the_projects_poisson():
    """grid_operator with c = 1, s = 0 is tools.poisson's matrix in its ordering"""
    A = grid_operator((5, 4), (1.0, 1.0), 0.0).toarray()
    n0 = 5
    for k in range(20):
        i0, i1 = k % n0, k // n0
        row = np.zeros(20)
        row[k] = 4.0
        if i0 > 0:
            row[k - 1] = -1.0
        if i0 < 4:
            row[k + 1] = -1.0
        if i1 > 0:
            row[k - n0] = -1.0
        if i1 < 3:
            row[k + n0] = -1.0
        assert np.array_equal(A[k], row)


def test_oracle_transfer_operators():
    P = _p1(7).toarray()
    assert P.shape == (7, 3) and np.array_equal(P[:, 1], [0, 0, 0.5, 1, 0.5, 0, 0]) and P[6, 2] == 0.5 and P[0, 0] == 0.5
    P = _p1(8).toarray()
    assert P.shape == (8, 4) and np.array_equal(P[:, 3], [0, 0, 0, 0, 0, 0, 0.5, 1.0])
    O = oracle_for((9, 8, 7))
    assert np.isclose(O.R[0].toarray().sum(axis=1).max(), 1.0)  # full weighting: an interior row sums to one
    # semi-coarsening: an axis shorter than 4 keeps the identity
    O = oracle_for((8, 3))
    assert O.P[0].shape == (24, 12) and O.grids == [(8, 3), (4, 3), (2, 3)]


CASES = [((7,), None, 0.0), ((64,), None, 0.0), ((5, 4), None, 0.0), ((37, 50), None, 0.0), ((9, 8, 7), None, 0.0),
         ((3, 3, 3), None, 0.0), ((16, 16, 3), None, 0.0), ((37, 50), (2.5, 0.7), 0.3),
         ((10, 12, 14), (4.0, 1.0, 0.5), 0.01)]


@pytest.mark.parametrize("grid,c,s", CASES)
@pytest.mark.parametrize("omega,steps", [(0.8, 2), (1.0, 1), (2.0 / 3.0, 3)])
def test_oracle_cycle_is_symmetric_positive_definite(grid, c, s, omega, steps):
    O = oracle_for(grid, c, s)
    n = int(np.prod(grid))
    rng = np.random.default_rng(n)
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = O.apply(u, omega, steps), O.apply(v, omega, steps)
        assert abs(u @ Mv - v @ Mu) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(Mv)
        assert u @ Mu > 0.0 and v @ Mv > 0.0


def test_oracle_preconditioned_pcg_counts_do_not_grow_with_the_grid():
    """the reason for the feature: Jacobi-PCG needs O(n_axis) iterations, the V-cycle about ten"""
    counts = {}
    for grid, c, s in (((37, 50), None, 0.0), ((130, 67), None, 0.0), ((37, 50), (2.5, 0.7), 0.3)):
        O = oracle_for(grid, c, s)
        A = O.A[0]
        b = np.random.default_rng(1).standard_normal(A.shape[0])
        x, it = numpy_pcg(A, b, 1e-8, 1000, O.apply)
        assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
        dinv = 1.0 / A.diagonal()
        _, itj = numpy_pcg(A, b, 1e-8, 1000, lambda r: dinv * r)
        counts[(grid, s)] = (it, itj)
        assert 5 <= it <= 14 and itj >= 4 * it, counts
