"""CPU: precon.multigrid(..., galerkin=True, line=a) / device.DeviceMultigridLine -- the new keyword and its refusals before
any device call, the new C symbols, and the oracle of the line-smoothed Galerkin V-cycle: the level
lists (the line axis is never coarsened, every other axis is halved down to 1), the level operators R A P from SciPy
products, the Thomas solves vectorised over the grid lines in exactly section 9h's order, the cycle in float64 and the same
cycle in np.longdouble as the yardstick of both.  tests/test_gpu_multigrid_line.py imports the oracle, the operator
generator and the case lists from here.  Nothing here needs a GPU.

The tests under "the feature" exercise the library and fail without it.  The tests under "oracle guards" (level lists,
symmetry and definiteness of the dense cycle, the two legs against each other, the PCG counts that are the reason for the
feature) guard the yardstick, not the code: they pass whatever the library does, and are here so that a mistake in the
oracle cannot pass for one in the kernels."""
import functools
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _p1, numpy_pcg
from test_multigrid_galerkin_host import GalerkinOracle, _LdMat, _ld_triple, varying_operator

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# ------------------------------------------------------------------------------------------------ the test operators


def widths(n, ratio=1.0, scale=1.0, both_ends=False):
    """cell widths along one axis: uniform 1 / n, or graded h_i ~ ratio^(i / (n - 1)) normalised to sum 1 (both_ends: graded
    from the middle towards both ends, the finest cells at the ends); `scale` stretches the axis as a whole"""
    if ratio == 1.0 or n == 1:
        h = np.full(n, 1.0 / n)
    else:
        i = np.arange(n, dtype=np.float64)
        if both_ends:
            i = np.minimum(i, n - 1 - i) * 2.0
        h = ratio ** (i / (n - 1))
        h = h / h.sum()
    return h * scale


def _t1_mesh(h):
    """the 1-D finite-volume Laplacian on cells of widths h: face weights t_0 = 2 / h_0, t_i = 2 / (h_{i-1} + h_i),
    t_n = 2 / h_{n-1}; tridiag(-t_i, t_i + t_{i+1}, -t_{i+1})"""
    n = h.size
    t = np.empty(n + 1)
    t[0], t[n] = 2.0 / h[0], 2.0 / h[n - 1]
    t[1:n] = 2.0 / (h[:-1] + h[1:])
    return sp.diags([-t[1:n], t[:-1] + t[1:], -t[1:n]], [-1, 0, 1], format="csr")


def mesh_operator(hs):
    """A = sum_a (x)_b (T1_a if b = a else diag(h_b)) on the tensor mesh with cell widths hs[a] along axis a, axis 0 the
    fastest index; an axis of one cell has no couplings and adds nothing.  Exactly symmetric."""
    A = None
    for a, h in enumerate(hs):
        if h.size == 1:
            continue
        T = _kron_axes([_t1_mesh(hb) if b == a else sp.diags([hb], [0], format="csr") for b, hb in enumerate(hs)])
        A = T if A is None else A + T
    A = A.tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def graded_operator(grid, axis, ratio=1.0, scale=1.0, both_ends=False):
    """the mesh operator on `grid` with uniform cells but along `axis`, which is graded (ratio) or stretched (scale)"""
    return mesh_operator([widths(m, ratio, scale, both_ends) if a == axis else widths(m) for a, m in enumerate(grid)])


def rhs(n):
    return np.random.default_rng(3).random(n)


# ------------------------------------------------------------------------------------------------ the oracle

def line_level_grids(grid, line):
    """section 9h: the line axis is never coarsened, every other axis is halved while it has at least 2 points"""
    out = [tuple(int(g) for g in grid)]
    while any(g >= 2 for a, g in enumerate(out[-1]) if a != line):
        out.append(tuple(g // 2 if (a != line and g >= 2) else g for a, g in enumerate(out[-1])))
    return out


def _line_parts(rows, cols, vals, g, line):
    """(d, l) of the line operator of a level from its sorted COO triples, as arrays of shape (n_line, lines): d the
    diagonal, l[i] = A[K_i, K_i - st_a] (l[0] = 0)"""
    n = int(np.prod(g))
    st = int(np.prod(g[:line]))
    ia = (rows // st) % g[line]
    d = np.zeros(n, dtype=vals.dtype)
    l = np.zeros(n, dtype=vals.dtype)
    m = rows == cols
    d[rows[m]] = vals[m]
    m = (cols == rows - st) & (ia >= 1)
    l[rows[m]] = vals[m]
    return _to_lines(d, g, line), _to_lines(l, g, line)


def _to_lines(v, g, line):
    """a level vector as (n_line, lines): axis 0 of the grid is the last NumPy axis"""
    nd = len(g)
    return np.moveaxis(v.reshape(g[::-1]), nd - 1 - line, 0).reshape(g[line], -1)


def _from_lines(V, g, line):
    nd = len(g)
    shape = list(g[::-1])
    m = shape.pop(nd - 1 - line)
    return np.moveaxis(V.reshape([m] + shape), 0, nd - 1 - line).reshape(-1)


def _factor(d, l):
    """p_0 = d_0, p_i = d_i - l_i (l_i q_{i-1}), q_i = 1 / p_i, every line at once"""
    q = np.empty_like(d)
    one = d.dtype.type(1)
    q[0] = one / d[0]
    for i in range(1, d.shape[0]):
        q[i] = one / (d[i] - l[i] * (l[i] * q[i - 1]))
    return q


def _solve(q, l, r):
    """e = T^-1 r: y_0 = r_0, y_i = r_i - (l_i q_{i-1}) y_{i-1}; e_{n-1} = q_{n-1} y_{n-1}, e_i = q_i (y_i - l_{i+1} e_{i+1})"""
    n = q.shape[0]
    y = np.empty_like(r)
    y[0] = r[0]
    for i in range(1, n):
        y[i] = r[i] - (l[i] * q[i - 1]) * y[i - 1]
    e = np.empty_like(r)
    e[n - 1] = q[n - 1] * y[n - 1]
    for i in range(n - 2, -1, -1):
        e[i] = q[i] * (y[i] - l[i + 1] * e[i + 1])
    return e


class LineOracle:
    """the levels of one operator with line axis `line`: A_0 = A, A_{l+1} = R_l A_l P_l with section 9c's P_a on every axis
    but `line` and R_l = P_l' / 2^(coarsened axes), the factors q of the line operators -- in float64 from SciPy (apply) and
    in np.longdouble (apply_ext; built on first use)"""

    def __init__(self, grid, line, A):
        assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended format here: the yardstick is missing"
        self.grid, self.line = tuple(int(g) for g in grid), int(line)
        self.grids = line_level_grids(self.grid, self.line)
        self.A, self.P, self.R, self.scale = [A.tocsr()], [], [], []
        for g in self.grids[:-1]:
            co = [a != self.line and m >= 2 for a, m in enumerate(g)]
            P = _kron_axes([_p1(m) if k else sp.identity(m, format="csr") for m, k in zip(g, co)]).tocsr()
            scale = 1.0 / 2.0 ** sum(co)
            R = (P.T * scale).tocsr()
            self.P.append(P)
            self.R.append(R)
            self.scale.append(scale)
            Ac = (R @ self.A[-1] @ P).tocsr()
            Ac.sort_indices()
            self.A.append(Ac)
        self.q, self.l = [], []
        for g, M in zip(self.grids, self.A):
            C = M.tocoo()
            d, l = _line_parts(C.row, C.col, C.data, g, self.line)
            self.l.append(l)
            self.q.append(_factor(d, l))
        self._ext = None

    def solve(self, level, r):
        g = self.grids[level]
        return _from_lines(_solve(self.q[level], self.l[level], _to_lines(r, g, self.line)), g, self.line)

    def apply(self, b, omega=0.8, steps=2, level=0):
        if level == len(self.grids) - 1:
            return self.solve(level, b)
        A = self.A[level]
        x = np.zeros_like(b)
        for _ in range(steps):
            x = x + omega * self.solve(level, b - A @ x)
        x = x + self.P[level] @ self.apply(self.R[level] @ (b - A @ x), omega, steps, level + 1)
        for _ in range(steps):
            x = x + omega * self.solve(level, b - A @ x)
        return x

    def ext(self):
        """(Ax, Px, Rx, qx, lx): the longdouble leg's levels"""
        if self._ext is None:
            Ax, Px, Rx, qx, lx = [_LdMat.from_scipy(self.A[0])], [], [], [], []
            for P, R, s in zip(self.P, self.R, self.scale):
                Px.append(_LdMat.from_scipy(P))
                Rx.append(_LdMat.from_scipy(R))
                Ax.append(_ld_triple(Ax[-1], P, s))
            for g, M in zip(self.grids, Ax):
                d, l = _line_parts(M.rows, M.cols, M.vals, g, self.line)
                lx.append(l)
                qx.append(_factor(d, l))
            self._ext = (Ax, Px, Rx, qx, lx)
        return self._ext

    def apply_ext(self, b, omega=0.8, steps=2, level=0):
        Ax, Px, Rx, qx, lx = self.ext()
        b = np.asarray(b, dtype=LD)
        g = self.grids[level]

        def solve(r):
            return _from_lines(_solve(qx[level], lx[level], _to_lines(r, g, self.line)), g, self.line)

        if level == len(self.grids) - 1:
            return solve(b)
        A, w = Ax[level], LD(omega)
        x = np.zeros_like(b)
        for _ in range(steps):
            x = x + w * solve(b - A.dot(x))
        x = x + Px[level].dot(self.apply_ext(Rx[level].dot(b - A.dot(x)), omega, steps, level + 1))
        for _ in range(steps):
            x = x + w * solve(b - A.dot(x))
        return x


@functools.lru_cache(maxsize=None)
def line_oracle_for(grid, line, ratio=1.0, scale=1.0, both_ends=False, axis=None):
    """the oracle of the mesh operator graded / stretched along `axis` (default: the line axis itself)"""
    grid = tuple(grid)
    return LineOracle(grid, line, graded_operator(grid, line if axis is None else axis, ratio, scale, both_ends))


@functools.lru_cache(maxsize=None)
def line_oracle_kappa(grid, line, kind):
    """... of the cell-varying kappa operator of tests/test_multigrid_galerkin_host.py"""
    grid = tuple(grid)
    return LineOracle(grid, line, varying_operator(grid, kind))


# the table of the issue (CPU prototype): operator -> (point-smoothed Galerkin cycle, line cycle) PCG iterations to 1e-8
# on b = default_rng(3).random(n), omega = 0.8, steps = 2.  (grid, line, ratio, scale, both_ends)
TABLE = [
    ((32, 32, 32), 2, 1.0, 1.0, False, 8, 6),
    ((32, 32, 32), 2, 100.0, 1.0, False, 25, 6),
    ((32, 32, 32), 2, 1.0e4, 1.0, False, 33, 6),
    ((32, 32, 32), 2, 1.0, 1.0 / 20.0, False, 59, 4),
    ((32, 32, 32), 2, 1.0, 20.0, False, 56, 7),
    ((21, 37, 45), 2, 1.0e3, 1.0, False, 49, 10),
    ((24, 40, 20), 1, 1.0e3, 1.0, False, 42, 7),
    ((64, 64), 1, 1.0e3, 1.0, False, 49, 6),
    ((64, 64), 1, 300.0, 1.0, True, 29, 6),
]
# the four graded cases the GPU test solves with both handles: the line count is at most a third of the point count
GRADED = [((32, 32, 32), 2, 1.0e4), ((21, 37, 45), 2, 1.0e3), ((24, 40, 20), 1, 1.0e3), ((64, 64), 1, 1.0e3)]


@functools.lru_cache(maxsize=None)
def pcg_counts(grid, line, ratio=1.0, scale=1.0, both_ends=False, point=True):
    """(PCG iterations with the point-smoothed Galerkin oracle or None, with the line oracle) to 1e-8"""
    O = line_oracle_for(grid, line, ratio, scale, both_ends)
    A = O.A[0]
    b = rhs(A.shape[0])
    x, itl = numpy_pcg(A, b, 1e-8, 500, O.apply)
    assert np.linalg.norm(b - A @ x) <= 2e-8 * np.linalg.norm(b)
    itp = numpy_pcg(A, b, 1e-8, 500, GalerkinOracle(grid, A).apply)[1] if point else None
    return itp, itl


# ------------------------------------------------------------------------------------------------ the feature

def ll(n, m=None):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, m or n)
    for i in range(min(n, m or n)):
        A[i, i] = 2.0
    return A


def fake_csr(shape):
    from pysparse_amd import device

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing may reach the library
            self._h = None
            self.shape = shape

    return FakeCSR(shape)


def test_precon_multigrid_takes_the_keyword():
    """(there is no device here: a call that passed every check would raise RuntimeError, not ValueError)"""
    from pysparse.precon import precon
    import pysparse_amd.precon.precon as p2
    assert precon.multigrid is p2.multigrid and "line=None" in precon.multigrid.__doc__
    # a valid axis passes the parser: what surfaces is the ValueError of a later check, which does not name the keyword
    with pytest.raises(ValueError, match="omega") as e:
        precon.multigrid(ll(6), (2, 3), omega=2.0, galerkin=True, line=1)
    assert "line" not in str(e.value)
    with pytest.raises(ValueError, match="omega"):
        precon.multigrid(ll(6), (2, 3), omega=2.0, galerkin=True, line=None)
    with pytest.raises(TypeError):  # a keyword, not a seventh positional argument
        precon.multigrid(ll(6), (2, 3), 0.8, 2, True, "double", 1)


def test_device_layer_has_the_class():
    from pysparse_amd import device
    assert issubclass(device.DeviceMultigridLine, device.DeviceMultigrid)
    p = inspect.signature(device.DeviceMultigridLine.__init__).parameters
    assert list(p)[1:] == ["A", "grid", "omega", "steps", "galerkin", "line"] and p["line"].default is None
    with pytest.raises(ValueError, match="omega") as e:
        device.DeviceMultigridLine(fake_csr((6, 6)), (2, 3), omega=2.0, line=1)
    assert "line" not in str(e.value)


@pytest.mark.parametrize("bad", [True, False, 1.0, "1", (1,), np.float64(1.0)], ids=repr)
def test_a_line_that_is_no_int_is_a_type_error(bad):
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(TypeError, match="line"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, line=bad)
    with pytest.raises(TypeError, match="line"):
        device.DeviceMultigridLine(fake_csr((6, 6)), (2, 3), line=bad)


@pytest.mark.parametrize("grid,line,why", [
    ((2, 3), 2, "axes"), ((2, 3), -1, "axes"), ((1, 2, 3), 3, "axes"), ((2, 3), 2 ** 70, "axes"),   # outside 0 .. ND - 1
    ((6,), 0, "one axis"),                                                                            # ND = 1
    ((6, 1), 1, "at least 2"), ((1, 6), 0, "at least 2"), ((2, 1, 3), 1, "at least 2"),             # n_line < 2
])
def test_line_value_errors_before_any_device_call(grid, line, why):
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match=why):
        precon.multigrid(ll(6), grid, galerkin=True, line=line)
    if abs(line) < 2 ** 31:
        with pytest.raises(ValueError, match=why):
            device.DeviceMultigridLine(fake_csr((6, 6)), grid, line=line)


def test_line_needs_galerkin_and_double():
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match="galerkin=True"):
        precon.multigrid(ll(6), (2, 3), line=1)
    with pytest.raises(ValueError, match="galerkin=True"):
        precon.multigrid(ll(6), (2, 3), galerkin=False, line=0)
    with pytest.raises(ValueError, match="galerkin=True"):
        device.DeviceMultigridLine(fake_csr((6, 6)), (2, 3), galerkin=False, line=1)
    with pytest.raises(ValueError, match="single-precision"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, precision="single", line=1)


@pytest.mark.parametrize("n,m,args", [
    (6, 6, ((),)), (6, 6, ((1, 1, 2, 3),)), (6, 6, ((0, 6),)), (6, 6, ((2, 2),)), (6, 5, ((2, 3),)),
    (6, 6, ((2, 3), 0.0)), (6, 6, ((2, 3), 1.0000001)), (6, 6, ((2, 3), 0.8, 0)),
])
def test_everything_galerkin_refuses_is_refused_with_line(n, m, args):
    from pysparse.precon import precon
    with pytest.raises(ValueError):
        precon.multigrid(ll(n, m), *args, galerkin=True, line=0)
    with pytest.raises(TypeError):
        precon.multigrid(ll(6), 6, galerkin=True, line=0)


NEW_SYMBOLS = ("psp_mg_create_csr_line", "psp_mg_create_sss_line", "psp_mg_line_axis")


def test_new_symbols_are_declared_and_exported():
    from pysparse_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pysparse_hip.h")) as f:
        header = f.read()
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in _capi.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name  # bound with a signature, not only exported


# ------------------------------------------------------------------------------------------------ oracle guards

def test_extended_precision_is_there():
    """fails, not skips: without an extended format the yardstick of the GPU test would be float64 itself"""
    assert np.finfo(LD).eps < 1e-18


def test_level_lists():
    assert line_level_grids((5, 6, 9), 2) == [(5, 6, 9), (2, 3, 9), (1, 1, 9)]           # 3 -> 1 and 2 -> 1
    assert line_level_grids((7, 12), 1) == [(7, 12), (3, 12), (1, 12)]
    assert line_level_grids((1, 40), 1) == [(1, 40)]
    assert line_level_grids((300, 3), 1) == [(300, 3), (150, 3), (75, 3), (37, 3), (18, 3), (9, 3), (4, 3), (2, 3), (1, 3)]
    assert line_level_grids((3, 2100), 1) == [(3, 2100), (1, 2100)]
    assert line_level_grids((33, 17, 65), 0) == [(33, 17, 65), (33, 8, 32), (33, 4, 16), (33, 2, 8), (33, 1, 4), (33, 1, 2),
                                                 (33, 1, 1)]
    assert line_level_grids((33, 17, 65), 1)[-1] == (1, 17, 1) and line_level_grids((33, 17, 65), 2)[-1] == (1, 1, 65)
    assert line_level_grids((70, 70, 5), 2) == [(70, 70, 5), (35, 35, 5), (17, 17, 5), (8, 8, 5), (4, 4, 5), (2, 2, 5),
                                                (1, 1, 5)]
    O = line_oracle_for((5, 6, 9), 2, 1.0e4)
    assert [M.shape[0] for M in O.A] == [270, 54, 9]
    # on the last level A is its own line operator: the cycle there is exact
    d, l = _line_parts(*(lambda C: (C.row, C.col, C.data))(O.A[-1].tocoo()), O.grids[-1], 2)
    T = sp.diags([l[1:, 0], d[:, 0], l[1:, 0]], [-1, 0, 1])
    assert abs(T - O.A[-1]).max() == 0.0


def test_mesh_operator():
    """uniform widths give the project's Poisson operator up to the cell volume; graded widths are seeded by nothing, exactly
    symmetric, positive on the diagonal and carry the axis pattern only"""
    from test_multigrid_host import grid_operator
    A = graded_operator((5, 6, 9), 2)
    h = (1 / 5, 1 / 6, 1 / 9)
    c = [h[(a + 1) % 3] * h[(a + 2) % 3] / h[a] for a in range(3)]
    B = grid_operator((5, 6, 9), c, 0.0)
    C = A.tocoo()
    inner = np.abs(C.row - C.col) > 0
    Bc = B.tocsr()
    assert np.abs(C.data[inner] - np.asarray(Bc[C.row[inner], C.col[inner]]).ravel()).max() <= 1e-13 * abs(B).max()
    for grid, axis, ratio in (((5, 6, 9), 2, 1.0e4), ((7, 12), 1, 1.0e3), ((33, 17, 65), 0, 1.0e4)):
        A = graded_operator(grid, axis, ratio)
        assert abs(A - A.T).max() == 0.0 and A.diagonal().min() > 0.0
        C = A.tocoo()
        assert set(np.abs(C.col - C.row)) <= set(np.cumprod((1,) + grid[:-1])) | {0}
        hw = widths(grid[axis], ratio)
        assert abs(hw.sum() - 1.0) <= 1e-14 and abs(hw[-1] / hw[0] - ratio) <= 1e-9 * ratio


@pytest.mark.parametrize("grid,line", [((5, 6, 9), 2), ((7, 12), 1)])
def test_the_dense_cycle_is_symmetric_positive_definite(grid, line):
    n = int(np.prod(grid))
    for ratio in (1.0, 1.0e4):
        O = line_oracle_for(grid, line, ratio)
        for omega, steps in ((0.8, 2), (1.0, 1), (0.5, 3)):
            M = np.column_stack([O.apply(e, omega, steps) for e in np.eye(n)])
            assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
            assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0


@pytest.mark.parametrize("grid,line", [((5, 6, 9), 2), ((7, 12), 1), ((1, 40), 1), ((300, 3), 1), ((3, 2100), 1),
                                       ((33, 17, 65), 0)])
def test_the_two_legs_agree(grid, line):
    """the float64 leg against the extended one (what the GPU test's bound is measured in).  Each step of the cycle solves
    a system of a level exactly or smooths it, and a level's condition is at most of the order of max(n_a)^2 for these
    mesh Laplacians: the float64 leg's own error grows with it -- a few eps on the small grids, 1.1e3 eps on (300, 3)
    (nine levels along the axis of 300) and 1.4e4 eps on (3, 2100) (Thomas over 2100 points), measured.  The bound here is
    64 eps up to 16 points per axis and grows with max(n_a)^2 beyond: it catches a leg that computes something else, the
    GPU test takes e64 itself as its unit."""
    for ratio in (1.0, 1.0e4):
        O = line_oracle_for(grid, line, ratio)
        b = np.random.default_rng(3).standard_normal(int(np.prod(grid)))
        z, zx = O.apply(b), O.apply_ext(b)
        assert zx.dtype == LD
        e64 = float(np.abs(z - zx).max() / np.abs(zx).max())
        print(grid, line, ratio, "e64 = %.1f eps" % (e64 / EPS))
        assert e64 <= 64 * EPS * max(1.0, (max(grid) / 16.0) ** 2)


def test_a_single_level_is_the_exact_inverse():
    O = line_oracle_for((1, 40), 1, 1.0e4)
    x = np.random.default_rng(5).standard_normal(40)
    zx = O.apply_ext(O.ext()[0][0].dot(x.astype(LD)))
    assert np.abs(zx - x).max() <= 1e-13 * np.abs(x).max()


@pytest.mark.parametrize("grid,line,ratio,scale,both,point,lines", TABLE,
                         ids=["%s-l%d-r%g-s%g%s" % ("x".join(map(str, t[0])), t[1], t[2], t[3], "-both" if t[4] else "")
                              for t in TABLE])
def test_oracle_pcg_counts(grid, line, ratio, scale, both, point, lines):
    """the reason for the feature, as counted by the CPU prototype: the point-smoothed cycle loses its grid-independent
    convergence on a graded or stretched axis, the line cycle keeps it"""
    itp, itl = pcg_counts(grid, line, ratio, scale, both)
    print(grid, line, ratio, scale, both, "point", itp, "line", itl)
    assert (itp, itl) == (point, lines)
