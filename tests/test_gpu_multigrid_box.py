"""GPU: precon.multigrid(..., galerkin=True, stencil='box') / device.DeviceMultigridBox (psp_mg.hip, psp_mg_galerkin.h;
DESIGN.md section 9i) against the oracle and the operators of tests/test_multigrid_box_host.py.

The grids are the smallest at which each path can go wrong: (3, 3) a single level, the dense solve only; (4, 4) and (2, 9)
n0 = 2, where the flat offsets +1 and (-1, +1) coincide; (7, 12), (33, 17) odd and even lengths over two restriction tiles
along axis 0; (4, 4, 4), (5, 6, 9); (9, 3, 8) an axis that is never coarsened; (8, 1, 8) an axis of length 1 inside a 3-D
grid; (40, 36, 20) more than one restriction tile in every direction and two levels above the tail; (16, 16, 16) and
(64, 64) for the solves.  The largest has 28 800 points.

Bounds (the rules of tests/test_gpu_multigrid_galerkin.py and tests/test_gpu_multigrid_single.py, copied).  A level operator
entry: 2 * 3^(2 ND) eps (R |A| P)[K, J].  One application: max(64 eps, 8 e64) max|z_ext| with z_ext the cycle in
np.longdouble and e64 the float64 SciPy oracle's own distance from it.  One single-precision application:
max(64 eps32, 8 e32) max|z_ext| with e32 the float32 NumPy leg's distance.  PCG with the double handle takes exactly the
iterations of the host file's table; with the single-precision handle those of NumPy PCG with the float32 leg, +-1."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _p1, level_grids, numpy_pcg
from test_multigrid_galerkin_host import varying_operator
from test_multigrid_single_host import EPS32, Single, leg_distance
from test_multigrid_box_host import PCG_TABLE, box_operator, box_oracle_for, rhs
import test_gpu_multigrid_galerkin as gk

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GRIDS = [(3, 3), (4, 4), (2, 9), (7, 12), (33, 17), (4, 4, 4), (5, 6, 9), (9, 3, 8), (8, 1, 8), (40, 36, 20)]
# the lower offsets of the full pattern in the order the library stores them
FULL = {1: [(-1, 0, 0)],
        2: [(-1, 0, 0), (1, -1, 0), (0, -1, 0), (-1, -1, 0)],
        3: [(-1, 0, 0), (1, -1, 0), (0, -1, 0), (-1, -1, 0)] + [(d0, d1, -1) for d1 in (1, 0, -1) for d0 in (1, 0, -1)]}

gid = gk.gid


def kinds(grid):
    return ("q1kappa", "compact9") if len(grid) == 2 else ("q1kappa", "q1")


def cases(grids, extra=()):
    return [pytest.param(g, k, id="%s-%s" % (gid(g), k)) for g in grids for k in tuple(kinds(g)) + tuple(extra)]


@functools.lru_cache(maxsize=None)
def device_csr(grid, kind, seed=0):
    return gk.device_csr_from(box_oracle_for(grid, kind, seed).A[0])


def box(A, grid, omega=0.8, steps=2, **kw):
    from pysparse_amd import device as dev
    return dev.DeviceMultigridBox(A, grid, omega, steps, **kw)


def test_the_grids_reach_what_they_are_chosen_for():
    sizes = lambda g: [int(np.prod(l)) for l in level_grids(g)]  # noqa: E731
    assert len(level_grids((3, 3))) == 1
    assert sum(n > gk.TAIL_T for n in sizes((40, 36, 20))) == 2 and all(m > t for m, t in zip((20, 18, 10), (16, 4, 4)))
    assert all(g[1] == 3 for g in level_grids((9, 3, 8))) and all(g[1] == 1 for g in level_grids((8, 1, 8)))
    assert sizes((16, 16, 16))[0] > gk.TAIL_T and sizes((64, 64))[0] > gk.TAIL_T
    assert max(int(np.prod(g)) for g in GRIDS) == 28800


# ------------------------------------------------------------------------------------------------ structure

@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_structure(grid, steps):
    from pysparse_amd import device as dev
    A = device_csr(grid, "q1kappa")
    K = box(A, grid, 0.8, steps)
    lv, tail_first, launches = gk.expected_structure(grid, steps)
    info = K.info()
    assert K.levels == tuple(lv) and info["levels"] == len(lv)
    assert info["tail_first_level"] == tail_first and info["launches_per_apply"] == launches
    assert info["galerkin"] is True and info["stencil"] == "box" and info["line"] is None and info["precision"] == "double"
    assert K.stencil == "box"
    with pytest.raises(AttributeError):
        K.stencil = "axis"
    # every level, the finest included, holds the diagonal, omega / diagonal and all (3^nd - 1) / 2 lower arrays
    full = len(FULL[len(grid)])
    numbers = sum((2 + full) * int(np.prod(g)) for g in lv)
    b64 = K.bytes()
    assert 8 * numbers <= b64["operator"] < 8 * numbers + 16384  # the arrays, the tail's table and the dense inverse
    K32 = box(A, grid, 0.8, steps, precision="single")
    i32 = K32.info()
    assert i32.pop("precision") == "single" and info.pop("precision") == "double" and i32 == info
    assert 4 * numbers <= K32.bytes()["operator"] < 4 * numbers + 16384
    # an axis handle says so
    assert dev.DeviceMultigrid(dev.DeviceCSR.poisson(5, 4), (5, 4)).stencil == "axis"
    assert dev.DeviceMultigrid(dev.DeviceCSR.poisson(5, 4), (5, 4), galerkin=True).info()["stencil"] == "axis"


# ------------------------------------------------------------------------------------------------ level operators

@pytest.mark.parametrize("grid,kind", cases(GRIDS, ("axis7",)))
def test_level_operators(grid, kind):
    nd = len(grid)
    S = box_oracle_for(grid, kind).A[0]
    K = box(device_csr(grid, kind), grid)
    lv = level_grids(grid)
    assert K.levels == tuple(lv)
    offs, vals = K.level_operator(0)
    assert list(offs[1:]) == FULL[nd]
    prev = gk.assemble(grid, offs, vals)
    D = (prev - S).tocsr()
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0, "level 0 is not A bit for bit"
    assert np.array_equal(prev.diagonal(), S.diagonal())
    prev.eliminate_zeros()
    assert prev.nnz == S.nnz
    worst = 0.0
    for l in range(1, len(lv)):
        g = lv[l - 1]
        co = [m >= 4 for m in g]
        P = _kron_axes([_p1(m) if c else sp.identity(m, format="csr") for m, c in zip(g, co)]).tocsr()
        R = (P.T / 2.0 ** sum(co)).tocsr()
        offs, vals = K.level_operator(l)
        assert list(offs[1:]) == FULL[nd]
        cur = gk.assemble(lv[l], offs, vals)
        refs = (R @ prev @ P).tocsr()
        mag = (R @ abs(prev) @ P).tocsr()
        err = abs(cur - refs).tocsr()
        bound = 2.0 * 3 ** (2 * nd) * EPS * mag
        over = (err - bound).tocsr()
        assert over.nnz == 0 or over.data.max() <= 0.0, (grid, l, over.data.max())
        inv = mag.copy()
        inv.eliminate_zeros()
        inv.data = 1.0 / inv.data
        worst = max(worst, err.multiply(inv).max() / EPS)
        prev = cur
    print("grid %s %s: worst level-operator entry error %.2f eps (R|A|P), bound %d eps" % (grid, kind, worst, 2 * 3 ** (2 * nd)))
    K.close()


# ------------------------------------------------------------------------------------------------ one application

@pytest.mark.parametrize("grid,kind", cases(GRIDS, ("axis7",)))
def test_one_application_against_the_oracle(grid, kind):
    A, O = device_csr(grid, kind), box_oracle_for(grid, kind)
    worst = 0.0
    for omega in (0.8, 1.0):
        for steps in (1, 2):
            K = box(A, grid, omega, steps)
            b = rhs(grid, steps)
            z = np.full(b.size, np.nan)
            K.precon(b, z)
            zx = O.apply_ext(b, omega, steps)
            scale = float(np.abs(zx).max())
            e64 = float(np.abs(O.apply(b, omega, steps) - zx).max()) / scale
            err = float(np.abs(z - zx).max()) / scale
            bound = max(64.0 * EPS, 8.0 * e64)
            worst = max(worst, err / bound)
            print("grid %s %s omega %.1f steps %d: max|z - z_ext| = %.2f eps max|z_ext| (float64 oracle %.2f eps, bound %.1f eps, "
                  "ratio %.3f)" % (grid, kind, omega, steps, err / EPS, e64 / EPS, bound / EPS, err / bound))
            assert np.isfinite(z).all() and err <= bound, (grid, kind, omega, steps, err / EPS, bound / EPS)
            K.close()
    print("grid %s %s: worst ratio to the bound %.3f" % (grid, kind, worst))


@pytest.mark.parametrize("grid", [(7, 12), (5, 6, 9)], ids=gid)
def test_an_axis_operator_gives_what_the_axis_handle_gives_to_the_bound(grid):
    """a 5- / 7-point matrix passed with stencil='box': the sums run in another order, no bit claim -- both handles lie
    within the oracle bound of the same extended cycle"""
    from pysparse_amd import device as dev
    A, O = device_csr(grid, "axis7"), box_oracle_for(grid, "axis7")
    b = rhs(grid, 4)
    zx = O.apply_ext(b)
    scale = float(np.abs(zx).max())
    bound = max(64.0 * EPS, 8.0 * float(np.abs(O.apply(b) - zx).max()) / scale)
    for K in (box(A, grid), dev.DeviceMultigrid(A, grid, galerkin=True)):
        z = np.empty(b.size)
        K.precon(b, z)
        assert float(np.abs(z - zx).max()) / scale <= bound


# ------------------------------------------------------------------------------------------------ same bits

def blocks_equal_single(K, grid):
    """column c of a block application has the bits of the single application: k = 1, 3, 8 columns, from host blocks and
    from device blocks with a leading dimension above n"""
    from pysparse_amd import device as dev
    n, pad = int(np.prod(grid)), 5
    for k in (1, 3, 8):
        X = np.asfortranarray(np.random.default_rng(20 + k).standard_normal((n, k)))
        Y = np.full((n, k), np.nan, order="F")
        K.precon_block(X, Y)
        Xp = np.zeros((n + pad, k), order="F")
        Xp[:n] = X
        xd, yd = dev.DeviceBuffer.from_host(Xp.ravel(order="F")), dev.DeviceBuffer((n + pad) * k)
        yd.zero()
        K.precon_block_dev(k, xd.ptr, n + pad, yd.ptr, n + pad)
        Yp = yd.download().reshape((n + pad, k), order="F")
        assert not Yp[n:].any(), "the padding rows were written"
        for c in range(k):
            z = np.empty(n)
            K.precon(np.ascontiguousarray(X[:, c]), z)
            assert np.array_equal(Y[:, c], z) and np.array_equal(Yp[:n, c], z), (grid, k, c)


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_same_bits(grid, precision):
    from pysparse_amd import device as dev
    S = box_oracle_for(grid, "q1kappa").A[0]
    K = box(device_csr(grid, "q1kappa"), grid, precision=precision)
    b = rhs(grid, 3)
    z1, z2 = np.empty(b.size), np.empty(b.size)
    K.precon(b, z1)
    K.precon(b, z2)
    assert np.array_equal(z1, z2)
    xb, yb = dev.DeviceBuffer.from_host(b), dev.DeviceBuffer(b.size)
    yb.zero()
    K.precon_dev(xb.ptr, yb.ptr)
    assert np.array_equal(yb.download(), z1)
    assert np.array_equal(xb.download(), b)  # x is unchanged
    # an sss_mat handle of the same matrix, and a second csr handle built from scratch
    for other in (box(gk.device_sss_from(S), grid, precision=precision), box(gk.device_csr_from(S), grid, precision=precision)):
        assert other.info()["stencil"] == "box" and other.info()["precision"] == precision
        z3 = np.empty(b.size)
        other.precon(b, z3)
        assert np.array_equal(z3, z1)
        for l in range(len(K.levels)):
            assert np.array_equal(K.level_operator(l)[1], other.level_operator(l)[1])
    blocks_equal_single(K, grid)


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("grid", [(7,), (64,), (4100,)], ids=gid)
def test_a_one_dimensional_box_handle_is_the_axis_handle(grid, precision):
    """in 1-D the two patterns coincide: the same level operators and the same application, bit for bit"""
    from pysparse_amd import device as dev
    S = varying_operator(grid, "rand100", 0.3)
    A = gk.device_csr_from(S)
    Kb = box(A, grid, precision=precision)
    Ka = (dev.DeviceMultigrid32 if precision == "single" else dev.DeviceMultigrid)(A, grid, galerkin=True)
    assert (Kb.stencil, Ka.stencil) == ("box", "axis") and Kb.levels == Ka.levels
    ib, ia = Kb.info(), Ka.info()
    assert ib.pop("stencil") == "box" and ia.pop("stencil") == "axis" and ib == ia
    for l in range(len(Ka.levels)):
        ob, vb = Kb.level_operator(l)
        oa, va = Ka.level_operator(l)
        assert ob == oa and np.array_equal(vb, va)
    for omega, steps in ((0.8, 2), (1.0, 1)):
        Kb, Ka = box(A, grid, omega, steps, precision=precision), \
            (dev.DeviceMultigrid32 if precision == "single" else dev.DeviceMultigrid)(A, grid, omega, steps, galerkin=True)
        b = rhs(grid, 6)
        zb, za = np.full(b.size, np.nan), np.empty(b.size)
        Kb.precon(b, zb)
        Ka.precon(b, za)
        assert np.array_equal(zb, za)


# ------------------------------------------------------------------------------------------------ precision='single'

@pytest.mark.parametrize("grid,kind", cases(GRIDS))
def test_one_single_precision_application(grid, kind):
    A, O = device_csr(grid, kind), box_oracle_for(grid, kind)
    O32 = Single(O)
    K64 = box(A, grid)
    for omega, steps in ((0.8, 2), (1.0, 1)):
        K32 = box(A, grid, omega, steps, precision="single")
        b = rhs(grid, 1)
        z, z64 = np.full(b.size, np.nan), np.empty(b.size)
        K32.precon(b, z)
        K64.precon(b, z64)
        ref, e32 = leg_distance(O, O32, b, omega, steps)
        scale = float(np.abs(ref).max())
        err = float(np.abs(z - ref).max()) / scale
        bound = max(64.0 * EPS32, 8.0 * e32)
        print("grid %s %s omega %.1f steps %d: max|z - z_ref| = %.2f eps32 max|z_ref| (float32 leg %.2f eps32, bound %.1f eps32)"
              % (grid, kind, omega, steps, err / EPS32, e32 / EPS32, bound / EPS32))
        assert np.isfinite(z).all() and err <= bound, (grid, kind, omega, steps, err / EPS32, bound / EPS32)
        assert np.array_equal(z, z.astype(np.float32).astype(np.float64))  # what came out are floats, widened
        if b.size > 27:
            assert not np.array_equal(z, z64), "the single-precision handle gave the double handle's bits"
        K32.close()
    # the stored arrays are the double ones rounded once
    K32 = box(A, grid, precision="single")
    for l in range(len(K64.levels)):
        o32, v32 = K32.level_operator(l)
        o64, v64 = K64.level_operator(l)
        assert o32 == o64 and np.array_equal(v32, v64.astype(np.float32).astype(np.float64)), (grid, kind, l)


# ------------------------------------------------------------------------------------------------ solves

@pytest.mark.parametrize("kind,grid", sorted(PCG_TABLE), ids=lambda v: v if isinstance(v, str) else gid(v))
def test_pcg_takes_the_iterations_of_the_table(kind, grid):
    from pysparse_amd import device as dev
    seed, want, wantj = PCG_TABLE[(kind, grid)]
    A, O = device_csr(grid, kind), box_oracle_for(grid, kind)
    S = O.A[0]
    b = rhs(grid, seed)
    K = box(A, grid)
    x = np.zeros(b.size)
    info, it, relres = dev.pcg(A, b, x, 1e-8, 200, K)
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    xj = np.zeros(b.size)
    infoj, itj, _ = dev.pcg(A, b, xj, 1e-8, 5000, dev.DeviceJacobi(A))
    print("pcg %s %s: info %d, %d iterations (table: %d), true residual %.3e; Jacobi-PCG %d (table: %d)"
          % (kind, grid, info, it, want, res, itj, wantj))
    assert info == 0 and it == want and res <= 1e-8
    assert infoj == 0 and itj > it
    # the single-precision handle: the count of NumPy PCG with the float32 leg, within the margin of section 9g's tests
    it32 = numpy_pcg(S, b, 1e-8, 200, Single(O).apply)[1]
    x32 = np.zeros(b.size)
    info32, its, _ = dev.pcg(A, b, x32, 1e-8, 200, box(A, grid, precision="single"))
    res32 = np.linalg.norm(b - S @ x32) / np.linalg.norm(b)
    print("pcg %s %s precision='single': %d iterations (float32 leg: %d), true residual %.3e" % (kind, grid, its, it32, res32))
    assert info32 == 0 and abs(its - it32) <= 1 and res32 <= 2e-8


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("kind,grid", [("q1kappa", (64, 64)), ("q1kappa", (16, 16, 16))], ids=["64x64", "16x16x16"])
def test_pcg_batch_ends_each_column_as_the_single_solve(kind, grid, precision):
    from pysparse_amd import device as dev
    A = device_csr(grid, kind)
    n = int(np.prod(grid))
    K = box(A, grid, precision=precision)
    B = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 3)))
    X = np.zeros((n, 3), order="F")
    info, it, relres = dev.pcg_batch(A, B, X, 1e-8, 100, K)
    for c in range(3):
        x = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-8, 100, K)
        assert r[0] == 0 and (info[c], it[c]) == r[:2] and relres[c] == r[2]
        assert np.array_equal(X[:, c], x)


def test_the_drop_in_module_lobpcg_and_pcg():
    from pysparse.eigen import lobpcg
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    grid = (16, 16, 16)
    seed, want, _ = PCG_TABLE[("q1", grid)]
    S = box_oracle_for(grid, "q1").A[0]
    A = gk.ll_from(S).to_csr()
    K = precon.multigrid(A, grid, galerkin=True, stencil="box")
    assert K.stencil == "box" and K.galerkin is True and K.line is None and K.levels == tuple(level_grids(grid))
    assert precon.multigrid(A, grid, galerkin=True, stencil="box", precision="single").precision == "single"
    with pytest.raises(AttributeError):
        K.stencil = "axis"
    b = rhs(grid, seed)
    x = np.zeros(b.size)
    info, it, relres = krylov.pcg(A, b, x, 1e-8, 100, K)
    assert info == 0 and it == want and np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b)
    lam, Q, res, its = lobpcg.lobpcg(A, None, K, 3, 1e-8, 200)
    print("lobpcg k = 3 on %s: %d iterations, eigenvalues %s, residuals %s" % (grid, its, lam, res))
    assert np.all(np.asarray(res) <= 1e-8)
    R = S @ Q - Q * np.asarray(lam)
    assert np.linalg.norm(R, axis=0).max() <= 1e-6 * abs(S).max()
    # the axis default of the drop-in module: the same 27-point matrix is refused as before
    assert precon.multigrid(gk.ll_from(varying_operator((5, 4), "smooth")).to_csr(), (5, 4), galerkin=True).stencil == "axis"
    with pytest.raises(ValueError, match="no axis stride"):
        precon.multigrid(A, grid, galerkin=True)


# ------------------------------------------------------------------------------------------------ refusals

def symmetric_pair(S, i, j, v):
    P = S.tolil()
    P[i, j] = v
    P[j, i] = v
    P = P.tocsr()
    P.sort_indices()
    return P


def test_refusals_from_the_device_pass_name_their_kind():
    from pysparse_amd import device as dev

    def refused(M, grid, why, shape=None, **kw):
        if not isinstance(M, dev.DeviceCSR):
            M = gk.device_csr_from(M) if sp.issparse(M) else dev.DeviceCSR.from_arrays(shape, *M)
        with pytest.raises(ValueError, match=why) as e:
            box(M, grid, **kw)
        assert "stencil='box'" in str(e.value)

    grid = (7, 12)
    S = box_operator(grid, "q1kappa")
    box(gk.device_csr_from(S), grid).close()  # the unchanged matrix is accepted
    # an entry two points away along axis 0 (row 30 is (2, 4)), stored symmetrically; the same along axis 1
    refused(symmetric_pair(S, 30, 32, -1.0), grid, "offset")
    refused(symmetric_pair(S, 30, 44, -1.0), grid, "offset")
    refused(symmetric_pair(S, 30, 32, -1.0), grid, "offset", precision="single")
    # wrapped entries: the end of one grid line and the start of the next (flat offset +1), and the corner offset (+1, +1)
    # applied at a line end, which lands two lines further
    refused(symmetric_pair(S, 6, 7, -1.0), grid, "offset")
    refused(symmetric_pair(S, 6, 14, -1.0), grid, "offset")
    S29 = box_operator((2, 9), "q1kappa")
    box(gk.device_csr_from(S29), (2, 9)).close()
    assert S29[1, 2] != 0.0  # flat offset +1 from the line end (1, 0) IS the corner neighbour (0, 1) when n0 = 2 ...
    refused(symmetric_pair(S29, 1, 4, -1.0), (2, 9), "offset")  # ... and (+1, +1) from there wraps to (0, 2)
    # an unsymmetric pair: one direction of a corner coupling differs in the last bit, or is not stored at all
    assert S[30, 38] != 0.0
    P = S.copy()
    k = P.indptr[30] + list(P.indices[P.indptr[30]:P.indptr[31]]).index(38)
    P.data[k] = np.nextafter(P.data[k], 0.0)
    refused(P, grid, "unsymmetric")
    P = S.tolil()
    P[38, 30] = 0.0
    P = P.tocsr()
    P.eliminate_zeros()
    refused(P, grid, "unsymmetric")
    # a corner entry stored twice, through csr_from_arrays
    refused(gk.insert_entry(S, 30, 38, S[30, 38]), grid, "stored twice", shape=S.shape)
    # a missing, a zero and a negative diagonal entry
    at = S.indptr[40] + list(S.indices[S.indptr[40]:S.indptr[41]]).index(40)
    Z = S.copy()
    Z.data[at] = 0.0
    refused(Z, grid, "diagonal")
    Z = Z.copy()
    Z.eliminate_zeros()
    assert Z.nnz == S.nnz - 1
    refused(Z, grid, "diagonal")
    P = S.copy()
    P.data[at] = -1.0
    refused(P, grid, "diagonal")
    # the first kind in the order offset, duplicate, diagonal, symmetry is the one that is named
    refused(symmetric_pair(Z, 30, 32, -1.0), grid, "offset")
    # handles that are refused as today
    g3 = (9, 8, 7)
    rel = dev.DeviceCSR.poisson(*g3)
    rel.release_arrays()
    with pytest.raises(ValueError, match="index arrays"):
        box(rel, g3)
    with pytest.raises(ValueError):
        box(dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0]), (9, 8))


def test_the_same_matrices_without_the_keyword_are_refused_with_todays_text():
    from pysparse_amd import device as dev
    for grid, kind in (((7, 12), "q1kappa"), ((7, 12), "compact9"), ((5, 6, 9), "q1")):
        A = device_csr(grid, kind)
        for cls in (dev.DeviceMultigrid, dev.DeviceMultigrid32):
            with pytest.raises(ValueError, match="not a symmetric 3- / 5- / 7-point stencil on this grid: it has an entry at an "
                                                 "offset that is no axis stride of the grid"):
                cls(A, grid, galerkin=True)
            with pytest.raises(ValueError, match="constant-coefficient"):
                cls(A, grid)
    # the C ABI: the box bit without the Galerkin bit is refused, with either matrix
    import ctypes as C
    from pysparse_amd import _capi
    h, g = C.c_void_p(), (C.c_int * 2)(7, 12)
    for A in (device_csr((7, 12), "q1kappa"), dev.DeviceCSR.poisson(7, 12)):
        for flags in (dev.PSP_MG_BOX, dev.PSP_MG_BOX | dev.PSP_MG_SINGLE):
            assert _capi.lib().psp_mg_create_csr_ex(A._h, 2, g, 0.8, 2, flags, C.byref(h)) == -1 and h.value is None
            assert b"PSP_MG_GALERKIN" in _capi.lib().psp_last_error()
