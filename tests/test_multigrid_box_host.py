"""CPU: precon.multigrid(..., galerkin=True, stencil='box') / device.DeviceMultigridBox -- the keyword and its checks before
any device call, the new C symbols, the test operators with the full pattern {-1, 0, 1}^nd, and the PCG iteration counts
that tests/test_gpu_multigrid_box.py asserts.  The oracle is section 9d's: GalerkinOracle of
tests/test_multigrid_galerkin_host.py takes any symmetric SciPy matrix, with its float64 and its np.longdouble leg.
Nothing here needs a GPU.

The tests under "the feature" exercise the library and fail without it.  The tests under "oracle guards" guard the
yardstick, not the code.

The test operators, all with Dirichlet ends (the grid holds the interior nodes; an element that touches the boundary keeps
its interior nodes only):
  q1      K1 (x) M1 + M1 (x) K1 with K1 = tridiag(-1, 2, -1), M1 = tridiag(1, 4, 1) / 6: the bilinear Laplacian; in 3-D the
          trilinear one, K1 (x) M1 (x) M1 + M1 (x) K1 (x) M1 + M1 (x) M1 (x) K1
  q1kappa the same form assembled element by element with kappa per element, log-uniform in [1, 100], seeded
  compact9  the compact 9-point Laplacian (20, -4, -1) / 6 (2-D only)
  axis7   a 5- / 7-point operator of section 9d's tests (varying_operator 'rand100'), to be passed as a box operator"""
import functools
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _t1, level_grids
from test_multigrid_galerkin_host import GalerkinOracle, varying_operator

LD = np.longdouble
EPS = np.finfo(np.float64).eps
KINDS = ("q1", "q1kappa", "compact9", "axis7")

# ------------------------------------------------------------------------------------------------ the test operators


def _m1(n):
    return sp.diags([np.ones(n - 1), 4.0 * np.ones(n), np.ones(n - 1)], [-1, 0, 1], format="csr") / 6.0


def _s1(n):
    return sp.diags([np.ones(n - 1), np.ones(n - 1)], [-1, 1], shape=(n, n), format="csr")


def q1_operator(grid):
    grid = tuple(int(g) for g in grid)
    A = None
    for a in range(len(grid)):
        T = _kron_axes([_t1(m) if b == a else _m1(m) for b, m in enumerate(grid)])
        A = T if A is None else A + T
    return _finish(A)


def compact9_operator(grid):
    n0, n1 = grid
    I0, I1 = sp.identity(n0, format="csr"), sp.identity(n1, format="csr")
    A = (20.0 / 6.0) * _kron_axes([I0, I1]) - (4.0 / 6.0) * (_kron_axes([_s1(n0), I1]) + _kron_axes([I0, _s1(n1)])) \
        - (1.0 / 6.0) * _kron_axes([_s1(n0), _s1(n1)])
    return _finish(A)


def _finish(A):
    """sorted CSR without stored zeros, the upper triangle the mirror of the lower one bit for bit"""
    A = sp.csr_matrix(A)
    L = sp.tril(A, -1, format="csr")
    A = (L + L.T + sp.diags(A.diagonal())).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def kappa_cells(grid, seed=0):
    """kappa of every element, shape (grid + 1)[::-1]: a grid of n interior nodes along an axis has n + 1 elements"""
    rng = np.random.default_rng([seed, 9, len(grid)] + list(grid))
    return 10.0 ** rng.uniform(0.0, 2.0, tuple(int(g) + 1 for g in grid)[::-1])


def q1kappa_operator(grid, seed=0, kappa=None):
    """sum over the elements of kappa_e * (the element matrix of the form of q1_operator); element (e0, e1, e2) has the
    nodes e_a - 1 and e_a along axis a, those outside 0 .. n_a - 1 are boundary nodes and dropped"""
    grid = tuple(int(g) for g in grid)
    nd, n = len(grid), int(np.prod(grid))
    kap = kappa_cells(grid, seed) if kappa is None else kappa
    k1 = np.array([[1.0, -1.0], [-1.0, 1.0]])
    m1 = np.array([[2.0, 1.0], [1.0, 2.0]]) / 6.0
    Ke = np.zeros((2 ** nd, 2 ** nd))
    for a in range(nd):  # local node p = p0 + 2 p1 + 4 p2: axis 0 is the fastest index, as in _kron_axes
        T = np.ones((1, 1))
        for b in range(nd):
            T = np.kron(k1 if b == a else m1, T)
        Ke += T
    st = np.cumprod((1,) + grid[:-1])
    cells = np.indices(tuple(g + 1 for g in grid)[::-1])[::-1].reshape(nd, -1)  # cells[a] = e_a of every element
    kflat = kap.reshape(-1)
    rows, cols, vals = [], [], []
    for p in range(2 ** nd):
        for q in range(2 ** nd):
            ip = [cells[a] - 1 + ((p >> a) & 1) for a in range(nd)]
            iq = [cells[a] - 1 + ((q >> a) & 1) for a in range(nd)]
            ok = np.ones(kflat.size, dtype=bool)
            for a in range(nd):
                ok &= (ip[a] >= 0) & (ip[a] < grid[a]) & (iq[a] >= 0) & (iq[a] < grid[a])
            rows.append(sum(ip[a][ok] * st[a] for a in range(nd)))
            cols.append(sum(iq[a][ok] * st[a] for a in range(nd)))
            vals.append(kflat[ok] * Ke[p, q])
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    return _finish(A)


def box_operator(grid, kind, seed=0):
    grid = tuple(int(g) for g in grid)
    if kind == "q1":
        return q1_operator(grid)
    if kind == "q1kappa":
        return q1kappa_operator(grid, seed)
    if kind == "compact9":
        return compact9_operator(grid)
    if kind == "axis7":
        return varying_operator(grid, "rand100", 0.0, seed)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def box_oracle_for(grid, kind, seed=0):
    grid = tuple(grid)
    return GalerkinOracle(grid, box_operator(grid, kind, seed))


def rhs(grid, seed=0):
    return np.random.default_rng(seed).standard_normal(int(np.prod(grid)))


def pcg_margin(A, b, tol, maxit, precon):
    """the loop of the library's pcg (tests/test_multigrid_host.numpy_pcg) that also returns how far the recurrence residual
    of the last and of the last but one iteration are from the threshold: (iterations, ||r_last|| / (tol ||b||),
    ||r_before|| / (tol ||b||))"""
    x = np.zeros_like(b)
    r = b.copy()
    tolb = tol * np.linalg.norm(b)
    rho, p, before = 1.0, None, np.inf
    for it in range(1, maxit + 1):
        z = precon(r)
        rho1, rho = rho, r @ z
        p = z if it == 1 else z + (rho / rho1) * p
        q = A @ p
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        now = np.linalg.norm(r) / tolb
        if now <= 1.0:
            return it, now, before
        before = now
    return maxit + 1, now, before


# PCG to 1e-8 from x = 0 on b = rhs(grid, seed): (seed, iterations with the oracle's float64 cycle (omega 0.8, 2 steps),
# iterations with Jacobi), measured by test_the_table_is_what_the_oracle_gives below.  The seeds are the first from 11 on
# for which the recurrence residual of the V-cycle solve at its last iteration and at the one before, and that of the
# Jacobi solve at its last iteration, are more than 10 % away from tol ||b||, so that another rounding cannot move the
# count.  The GPU test asserts the V-cycle count exactly.
PCG_TABLE = {
    ("q1", (64, 64)): (11, 5, 139),
    ("q1kappa", (64, 64)): (25, 14, 218),
    ("compact9", (64, 64)): (11, 6, 161),
    ("q1", (16, 16, 16)): (11, 6, 36),
    ("q1kappa", (16, 16, 16)): (12, 8, 47),
    ("q1", (21, 13, 18)): (12, 6, 44),
    ("q1kappa", (21, 13, 18)): (12, 8, 50),
}


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


def test_stencil_is_a_keyword_and_documented():
    from pysparse.precon import precon
    assert "stencil='axis'" in precon.multigrid.__doc__ and "'box'" in precon.multigrid.__doc__
    with pytest.raises(TypeError):  # not a positional argument
        precon.multigrid(ll(6), (6,), 0.8, 2, True, "double", None, "box")


@pytest.mark.parametrize("bad", [1, None, b"box", True, ("box",)], ids=["int", "None", "bytes", "bool", "tuple"])
def test_a_stencil_that_is_no_str_is_a_type_error(bad):
    """(there is no device here: a call that reached the library would raise RuntimeError)"""
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(TypeError, match="stencil"):
        precon.multigrid(ll(6), (7,), galerkin=True, stencil=bad)  # before the grid is looked at
    with pytest.raises(TypeError, match="stencil"):
        device.DeviceMultigridBox(fake_csr((6, 6)), (7,), stencil=bad)


@pytest.mark.parametrize("bad", ["Box", "full", "9", ""])
def test_an_unknown_stencil_is_a_value_error(bad):
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match="stencil"):
        precon.multigrid(ll(6), (6,), galerkin=True, stencil=bad)
    with pytest.raises(ValueError, match="stencil"):
        device.DeviceMultigridBox(fake_csr((6, 6)), (6,), stencil=bad)


def test_box_needs_galerkin_and_takes_no_line():
    from pysparse.precon import precon
    from pysparse_amd import device
    for kw in ({}, {"galerkin": False}):
        with pytest.raises(ValueError, match="galerkin=True"):
            precon.multigrid(ll(6), (6,), stencil="box", **kw)
    with pytest.raises(ValueError, match="galerkin=True"):
        device.DeviceMultigridBox(fake_csr((6, 6)), (6,), galerkin=False)
    with pytest.raises(ValueError, match="not supported"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, line=0, stencil="box")
    with pytest.raises(ValueError, match="not supported"):
        device.DeviceMultigrid._create(object.__new__(device.DeviceMultigridBox), fake_csr((6, 6)), (2, 3), 0.8, 2, True, 0, "box")


@pytest.mark.parametrize("good,kw", [("axis", {}), ("axis", {"galerkin": True}), ("box", {"galerkin": True}),
                                     ("box", {"galerkin": True, "precision": "single"})])
def test_valid_strings_pass_the_parser(good, kw):
    """what surfaces is the ValueError of the later checks, which do not mention the keyword"""
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match="grid") as e:
        precon.multigrid(ll(6), (7,), stencil=good, **kw)
    assert "stencil" not in str(e.value)
    with pytest.raises(ValueError, match="omega"):
        precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2, stencil=good, **kw)
    if good == "box":
        with pytest.raises(ValueError, match="grid"):
            device.DeviceMultigridBox(fake_csr((6, 6)), (7,), **kw)
        with pytest.raises(ValueError, match="steps"):
            device.DeviceMultigridBox(fake_csr((6, 6)), (6,), 0.8, 0, **kw)


def test_device_multigrid_box():
    from pysparse_amd import device
    assert issubclass(device.DeviceMultigridBox, device.DeviceMultigrid)
    p = inspect.signature(device.DeviceMultigridBox.__init__).parameters
    assert list(p)[1:] == ["A", "grid", "omega", "steps", "galerkin", "stencil", "precision"]
    assert p["galerkin"].default is True and p["stencil"].default == "box" and p["precision"].default == "double"
    # DeviceMultigrid's signature is untouched
    assert list(inspect.signature(device.DeviceMultigrid.__init__).parameters)[1:] == ["A", "grid", "omega", "steps", "galerkin"]
    assert device.PSP_MG_BOX == 8 and device.PSP_MG_BOX not in (device.PSP_MG_GALERKIN, device.PSP_MG_SINGLE)
    assert isinstance(device.DeviceMultigrid.stencil, property) and device.DeviceMultigrid.stencil.fset is None
    with pytest.raises(TypeError, match="precision"):
        device.DeviceMultigridBox(fake_csr((6, 6)), (6,), precision=32)
    with pytest.raises(ValueError, match="precision"):
        device.DeviceMultigridBox(fake_csr((6, 6)), (6,), precision="half")


def test_the_drop_in_type_has_a_read_only_stencil():
    from pysparse.precon import precon
    d = precon.MultigridType.__dict__["stencil"]
    assert type(d).__name__ == "getset_descriptor" and "'axis' or 'box'" in d.__doc__


NEW_SYMBOLS = ("psp_mg_stencil",)


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
    assert "#define PSP_MG_BOX 8u" in header
    assert "int psp_mg_stencil(const psp_mg_t *K, int *box);" in header


# ------------------------------------------------------------------------------------------------ oracle guards

GUARD_GRIDS = [(5, 6), (4, 5, 6)]


def kinds_for(grid):
    return [k for k in KINDS if k != "compact9" or len(grid) == 2]


def test_extended_precision_is_there():
    assert np.finfo(LD).eps < 1e-18


@pytest.mark.parametrize("grid", [(3, 3), (2, 9), (7, 12), (5, 6, 9), (8, 1, 8)])
def test_operator_generators(grid):
    """exactly symmetric, positive diagonal, seeded, inside the box and (but for axis7) reaching its corners; with kappa = 1
    the element-by-element assembly is the Kronecker form"""
    nd = len(grid)
    for kind in kinds_for(grid):
        A = box_operator(grid, kind, 1)
        assert A.has_sorted_indices and abs(A - A.T).max() == 0.0 and A.diagonal().min() > 0.0
        assert abs(A - box_operator(grid, kind, 1)).max() == 0.0
        if kind in ("q1kappa", "axis7"):
            assert abs(A - box_operator(grid, kind, 2)).max() > 0.0
        C = A.tocoo()
        k, j, corner = C.row, C.col, np.zeros(C.nnz, dtype=int)
        for m in grid:
            assert np.abs(k % m - j % m).max() <= 1
            corner += (k % m != j % m)
            k, j = k // m, j // m
        want = sum(m > 1 for m in grid)
        assert corner.max() == (1 if kind == "axis7" else want)
        # (the trilinear Laplacian has no face couplings: 21 entries in a full row, not 27)
        assert np.diff(A.indptr).max() <= int(np.prod([min(m, 3) for m in grid]))
        assert np.linalg.eigvalsh(A.toarray()).min() > 0.0
    Q = q1_operator(grid)
    Kc = q1kappa_operator(grid, kappa=np.ones(tuple(g + 1 for g in grid)[::-1]))
    assert abs(Q - Kc).max() <= 8 * EPS * abs(Q).max()
    k = kappa_cells(grid, 3)
    assert 1.0 <= k.min() and k.max() <= 100.0


@pytest.mark.parametrize("grid", GUARD_GRIDS)
def test_oracle_cycle_is_symmetric_positive_definite(grid):
    """the dense cycle is symmetric to 1e-13 and all its eigenvalues are > 0"""
    n = int(np.prod(grid))
    for kind in kinds_for(grid):
        O = box_oracle_for(grid, kind)
        for omega, steps in ((0.8, 2), (1.0, 1)):
            M = np.column_stack([O.apply(e, omega, steps) for e in np.eye(n)])
            assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max(), (grid, kind)
            assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0, (grid, kind)


@pytest.mark.parametrize("grid", GUARD_GRIDS + [(7, 12), (9, 3, 8)])
def test_the_two_legs_agree(grid):
    for kind in kinds_for(grid):
        O = box_oracle_for(grid, kind)
        b = rhs(grid, 3)
        for omega, steps in ((0.8, 2), (1.0, 1)):
            z, zx = O.apply(b, omega, steps), O.apply_ext(b, omega, steps)
            assert zx.dtype == LD
            assert np.abs(z - zx).max() <= 64 * EPS * np.abs(zx).max(), (grid, kind)


@pytest.mark.parametrize("grid", [(33, 17), (5, 6, 9), (9, 3, 8)])
def test_level_operators_keep_the_box(grid):
    O = box_oracle_for(grid, "q1kappa")
    assert O.grids == level_grids(grid)
    for g, A in zip(O.grids, O.A):
        C = A.tocoo()
        k, j = C.row, C.col
        for m in g:
            assert np.abs(k % m - j % m).max() <= 1
            k, j = k // m, j // m


@pytest.mark.parametrize("kind,grid", sorted(PCG_TABLE), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_the_table_is_what_the_oracle_gives(kind, grid):
    seed, want, wantj = PCG_TABLE[(kind, grid)]
    O = box_oracle_for(grid, kind)
    A, b = O.A[0], rhs(grid, seed)
    it, last, before = pcg_margin(A, b, 1e-8, 200, O.apply)
    dinv = 1.0 / A.diagonal()
    itj, lastj, beforej = pcg_margin(A, b, 1e-8, 5000, lambda r: dinv * r)
    print("%s %s seed %d: V-cycle PCG %d iterations (stopping residual %.3f tol||b||, the one before %.3f), Jacobi PCG %d (%.3f, %.3f)"
          % (kind, grid, seed, it, last, before, itj, lastj, beforej))
    assert (it, itj) == (want, wantj)
    for r in (last, before, lastj):
        assert not 0.9 <= r <= 1.1, "a residual within 10 % of the threshold: choose another seed"
    assert it <= 20 and itj >= 4 * it
