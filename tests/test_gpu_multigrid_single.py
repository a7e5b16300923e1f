"""GPU: precon.multigrid(..., precision='single') / device.DeviceMultigrid32 (psp_mg.hip, psp_mg_galerkin.h; DESIGN.md
section 9g) against the float32 NumPy leg of tests/test_multigrid_single_host.py, whose case lists these tests run.

The grids are those of tests/test_gpu_multigrid_galerkin.py and the CASES of tests/test_gpu_multigrid.py: levels above the
tail, odd and even n0, n0 below any vector width, semi-coarsening, and the 1-D grid that is the float32 cycle's worst.

Bound of one application: max(64 eps32, 8 e32) max|z_ref|.  z_ref is the extended cycle (stored level operators) or the
float64 oracle (matrix-free), e32 the float32 NumPy leg's own distance from it.  64 is section 9c's asserted allowance for
two summation orders, in the unit of the arithmetic that runs; the second term is section 9d's rule.  The host file's
guard keeps e32 <= 8 eps32 on every case, so the bound is 64 eps32 throughout."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import level_grids, numpy_pcg, oracle_for
from test_multigrid_galerkin_host import GalerkinOracle, galerkin_oracle_for, varying_operator
from test_multigrid_single_host import (EPS32, G_GRIDS, G_KINDS, G_SHIFTS, MF_SOLVER_CASES, PARAMS, SEEDS, SOLVER_GRIDS,
                                        SOLVER_KINDS, Single, gid, leg_distance, mf_cases, pcg_counts, rhs, single_galerkin,
                                        single_mf)
import test_gpu_multigrid as mf
import test_gpu_multigrid_galerkin as gk

pytestmark = pytest.mark.gpu

MF_CASES, MF_IDS = mf_cases()
EINVAL = -1  # PSP_EINVAL


def handles(A, grid, omega=0.8, steps=2, galerkin=False):
    from pysparse_amd import device as dev
    return dev.DeviceMultigrid32(A, grid, omega, steps, galerkin=galerkin), dev.DeviceMultigrid(A, grid, omega, steps, galerkin=galerkin)


# ------------------------------------------------------------------------------------------------ one application

def check_applications(A, grid, O, O32, galerkin, tag):
    worst = 0.0
    for omega, steps in PARAMS:
        K32, K64 = handles(A, grid, omega, steps, galerkin)
        for seed in SEEDS:
            b = rhs(grid, seed)
            z, z64 = np.full(b.size, np.nan), np.empty(b.size)
            K32.precon(b, z)
            K64.precon(b, z64)
            ref, e32 = leg_distance(O, O32, b, omega, steps)
            scale = float(np.abs(ref).max())
            err = float(np.abs(z - ref).max()) / scale
            bound = max(64.0 * EPS32, 8.0 * e32)
            worst = max(worst, err / bound)
            print("%s omega %.4f steps %d seed %d: max|z - z_ref| = %.2f eps32 max|z_ref| (float32 leg %.2f eps32, bound %.1f eps32, "
                  "ratio %.3f)" % (tag, omega, steps, seed, err / EPS32, e32 / EPS32, bound / EPS32, err / bound))
            assert np.isfinite(z).all() and err <= bound, (tag, omega, steps, seed, err / EPS32, bound / EPS32)
            # what came out are floats, widened
            assert np.array_equal(z, z.astype(np.float32).astype(np.float64))
            if b.size > 27:
                assert not np.array_equal(z, z64), "the single-precision handle gave the double handle's bits"
        K32.close()
        K64.close()
    print("%s: worst ratio to the bound %.3f" % (tag, worst))


@pytest.mark.parametrize("s", G_SHIFTS)
@pytest.mark.parametrize("kind", G_KINDS)
@pytest.mark.parametrize("grid", G_GRIDS, ids=gid)
def test_one_application_galerkin(grid, kind, s):
    check_applications(gk.device_csr(grid, kind, s), grid, galerkin_oracle_for(grid, kind, s), single_galerkin(grid, kind, s), True,
                       "galerkin %s %s s %.1f" % (grid, kind, s))


@pytest.mark.parametrize("grid,c,s", MF_CASES, ids=MF_IDS)
def test_one_application_matrix_free(grid, c, s):
    check_applications(mf.device_csr(grid, c, s), grid, oracle_for(grid, c, s), single_mf(grid, c, s), False,
                       "matrix-free %s c %s s %s" % (grid, c, s))


# ------------------------------------------------------------------------------------------------ level operators

@pytest.mark.parametrize("kind", G_KINDS)
@pytest.mark.parametrize("grid", G_GRIDS, ids=gid)
def test_level_operators_are_the_double_ones_rounded(grid, kind):
    K32, K64 = handles(gk.device_csr(grid, kind, 0.3), grid, galerkin=True)
    assert K32.levels == K64.levels == tuple(level_grids(grid))
    for l in range(len(K64.levels)):
        o32, v32 = K32.level_operator(l)
        o64, v64 = K64.level_operator(l)
        assert o32 == o64
        assert v32.dtype == np.float64 and np.array_equal(v32, v64.astype(np.float32).astype(np.float64)), (grid, kind, l)


# ------------------------------------------------------------------------------------------------ same bits

def blocks_equal_single(K, grid, z_of):
    """column c of a block application has the bits of the single application: k = 1, 3, 8, 9 columns, from host blocks
    and from device blocks with a leading dimension above n"""
    from pysparse_amd import device as dev
    n, pad = int(np.prod(grid)), 5
    for k in (1, 3, 8, 9):
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
            z = z_of(np.ascontiguousarray(X[:, c]))
            assert np.array_equal(Y[:, c], z) and np.array_equal(Yp[:n, c], z), (grid, k, c)


def same_bits(K, A_sss, A_again, grid, galerkin):
    from pysparse_amd import device as dev
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
    K.precon_dev(xb.ptr, yb.ptr)
    assert np.array_equal(yb.download(), z1)
    Ks = dev.DeviceMultigrid32(A_sss, grid, galerkin=galerkin)
    K2 = dev.DeviceMultigrid32(A_again, grid, galerkin=galerkin)
    for other in (Ks, K2):
        assert other.info()["precision"] == "single" and other.info()["galerkin"] is galerkin
        z3 = np.empty(b.size)
        other.precon(b, z3)
        assert np.array_equal(z3, z1)
        if galerkin:
            for l in range(len(K.levels)):
                assert np.array_equal(K.level_operator(l)[1], other.level_operator(l)[1])

    def z_of(col):
        z = np.empty(col.size)
        K.precon(col, z)
        return z

    blocks_equal_single(K, grid, z_of)


@pytest.mark.parametrize("grid", G_GRIDS, ids=gid)
def test_same_bits_galerkin(grid):
    from pysparse_amd import device as dev
    S = galerkin_oracle_for(grid, "rand1e4", 0.3).A[0]
    K = dev.DeviceMultigrid32(gk.device_csr(grid, "rand1e4", 0.3), grid, galerkin=True)
    same_bits(K, gk.device_sss_from(S), gk.device_csr_from(S), grid, True)


@pytest.mark.parametrize("grid,c,s", MF_CASES, ids=MF_IDS)
def test_same_bits_matrix_free(grid, c, s):
    from pysparse_amd import device as dev
    S = mf.scipy_csr(grid, c, s)
    K = dev.DeviceMultigrid32(mf.device_csr(grid, c, s), grid)
    same_bits(K, gk.device_sss_from(S), mf.device_csr_from(S), grid, False)


# ------------------------------------------------------------------------------------------------ structure

@pytest.mark.parametrize("grid,galerkin", [(g, k) for g in G_GRIDS for k in (False, True)] + [((70, 66, 65), False)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_structure_and_bytes(grid, galerkin):
    from pysparse_amd import _capi
    A = gk.device_csr(grid, "smooth", 0.0) if galerkin else mf.device_csr(grid, None, 0.0)
    for steps in (1, 2, 3):
        K32, K64 = handles(A, grid, 0.8, steps, galerkin)
        i32, i64 = K32.info(), K64.info()
        assert i32.pop("precision") == "single" and i64.pop("precision") == "double"
        assert i32 == i64
        lv, tail_first, launches = gk.expected_structure(grid, steps)
        assert (i32["levels"], i32["tail_first_level"], i32["launches_per_apply"]) == (len(lv), tail_first, launches)
        bits = C.c_int()
        for K, want in ((K32, 32), (K64, 64)):
            assert _capi.lib().psp_mg_precision(K._h, C.byref(bits)) == 0 and bits.value == want
        b32, b64 = K32.bytes(), K64.bytes()
        print("%s galerkin %s steps %d: operator bytes %d / %d, vector bytes %d / %d (single / double)"
              % (grid, galerkin, steps, b32["operator"], b64["operator"], b32["vector"], b64["vector"]))
        assert 0 < b32["operator"] <= 0.5 * b64["operator"] + 4096 * len(lv)
        assert b32["vector"] <= b64["vector"]
        if galerkin:  # the stored arrays are counted: (2 + lower arrays) numbers per point of every level
            nd = len(grid)
            full = {1: 1, 2: 4, 3: 13}[nd]
            numbers = sum((2 + (nd if l == 0 else full)) * int(np.prod(g)) for l, g in enumerate(lv))
            assert b64["operator"] >= 8 * numbers and 4 * numbers <= b32["operator"] < 4 * numbers + 4096 * len(lv)
        K32.close()
        K64.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_the_single_precision_range_galerkin():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    S = varying_operator(grid, "smooth", 0.3)
    for scale in (1e39, 1e-40):
        T = S.copy()
        T.data = T.data * scale
        A = gk.device_csr_from(T)
        with pytest.raises(ValueError, match="single-precision range"):
            dev.DeviceMultigrid32(A, grid, galerkin=True)
        K = dev.DeviceMultigrid(A, grid, galerkin=True)  # the same matrix in double
        b = rhs(grid, 5)
        z = np.empty(b.size)
        K.precon(b, z)
        assert np.isfinite(z).all() and z.any()
    # the diagonal still fits, omega / diagonal falls below FLT_MIN
    T = S.copy()
    T.data = T.data * (3.0e38 / S.diagonal().max())
    assert np.float32(T.diagonal().max()) < np.inf
    with pytest.raises(ValueError, match="single-precision range"):
        dev.DeviceMultigrid32(gk.device_csr_from(T), grid, omega=0.01, galerkin=True)


def test_the_single_precision_range_matrix_free():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    for scale in (1e39, 1e-40):
        A = mf.device_csr_from(mf.scipy_csr(grid, (scale, scale, scale), 0.0))
        with pytest.raises(ValueError, match="single-precision range"):
            dev.DeviceMultigrid32(A, grid)
        K = dev.DeviceMultigrid(A, grid)
        b = rhs(grid, 5)
        z = np.empty(b.size)
        K.precon(b, z)
        assert np.isfinite(z).all() and z.any()


def test_refusals_of_the_double_modes_are_still_raised():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    S = varying_operator(grid, "smooth", 0.3)

    def refused(M, why, galerkin=True):
        if not isinstance(M, dev.DeviceCSR):
            M = gk.device_csr_from(M) if sp.issparse(M) else dev.DeviceCSR.from_arrays(S.shape, *M)
        with pytest.raises(ValueError, match=why):
            dev.DeviceMultigrid32(M, grid, galerkin=galerkin)

    P = S.tolil()
    P[8, 9] = -1.0
    P[9, 8] = -1.0
    P = P.tocsr()
    P.sort_indices()
    refused(P, "wraps across a line end")
    refused(gk.insert_entry(S, 100, 101, S[100, 101]), "stored twice")
    P = S.copy()
    k = P.indptr[200] + list(P.indices[P.indptr[200]:P.indptr[201]]).index(201)
    P.data[k] = np.nextafter(P.data[k], 0.0)
    refused(P, "unsymmetric")
    P = S.copy()
    P.data[S.indptr[300] + list(S.indices[S.indptr[300]:S.indptr[301]]).index(300)] = -1.0
    refused(P, "diagonal")
    refused(gk.insert_entry(S, 0, 300, 0.0), "no axis stride")
    rel = dev.DeviceCSR.poisson(*grid)
    rel.release_arrays()
    refused(rel, "index arrays")
    with pytest.raises(ValueError):
        dev.DeviceMultigrid32(dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0]), (9, 8), galerkin=True)
    # the matrix-free mode: a varying matrix, a perturbed value, a negative shift, positive couplings, a device list
    refused(S, "constant-coefficient", galerkin=False)
    C0 = mf.scipy_csr(grid, None, 0.0)
    P = C0.copy()
    P.data[P.indptr[200] + 1] *= 1.0 + 2.0 ** -40
    refused(P, "constant-coefficient", galerkin=False)
    refused(mf.scipy_csr(grid, None, -0.1), "shift", galerkin=False)
    with pytest.raises(ValueError, match="not negative"):
        dev.DeviceMultigrid32(mf.device_csr_from(mf.scipy_csr((9, 8), (-1.0, 1.0), 8.0)), (9, 8))
    with pytest.raises(ValueError):
        dev.DeviceMultigrid32(dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0]), (9, 8))
    with pytest.raises(ValueError):
        dev.DeviceMultigrid32(mf.device_csr(grid, None, 0.0), (8, 9, 7), omega=1.5)
    # unknown flag bits
    from pysparse_amd import _capi
    h, g = C.c_void_p(), (C.c_int * 3)(*grid)
    for flags in (4, 7, 1 << 31):
        assert _capi.lib().psp_mg_create_csr_ex(mf.device_csr(grid, None, 0.0)._h, 3, g, 0.8, 2, flags, C.byref(h)) == EINVAL
        assert h.value is None


# ------------------------------------------------------------------------------------------------ solvers

def solve_with(A, S, grid, K32, it32, tag):
    from pysparse_amd import device as dev
    b = rhs(grid, 11)
    x = np.zeros(b.size)
    info, it, relres = dev.pcg(A, b, x, 1e-8, 200, K32)
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    xj = np.zeros(b.size)
    infoj, itj, _ = dev.pcg(A, b, xj, 1e-8, 5000, dev.DeviceJacobi(A))
    print("pcg %s: info %d, %d iterations (NumPy PCG with the float32 leg: %d; Jacobi-PCG: %d), true residual %.3e"
          % (tag, info, it, it32, itj, res))
    assert info == 0 and res <= 2e-8
    assert abs(it - it32) <= 1
    assert infoj == 0 and 4 * it <= itj
    xm = np.zeros(b.size)
    infom, itm, _ = dev.minres(A, b, xm, 1e-8, 200, K32)
    resm = np.linalg.norm(b - S @ xm) / np.linalg.norm(b)
    print("minres %s: info %d, %d iterations, true residual %.3e" % (tag, infom, itm, resm))
    assert infom == 0 and resm <= 2e-8
    # the batched loop: each column ends as the single solve on the same handle
    n = b.size
    B = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 3)))
    X = np.zeros((n, 3), order="F")
    infob, itb, relb = dev.pcg_batch(A, B, X, 1e-8, 100, K32)
    for c in range(3):
        xc = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), xc, 1e-8, 100, K32)
        assert (infob[c], itb[c]) == r[:2] and relb[c] == r[2]
        assert np.array_equal(X[:, c], xc)


@pytest.mark.parametrize("kind", SOLVER_KINDS)
@pytest.mark.parametrize("grid", SOLVER_GRIDS, ids=gid)
def test_solvers_galerkin(grid, kind):
    from pysparse_amd import device as dev
    A, S = gk.device_csr(grid, kind, 0.0), galerkin_oracle_for(grid, kind, 0.0).A[0]
    solve_with(A, S, grid, dev.DeviceMultigrid32(A, grid, galerkin=True), pcg_counts("galerkin", grid, kind)[1],
               "galerkin %s %s" % (grid, kind))


@pytest.mark.parametrize("grid,c,s", MF_SOLVER_CASES)
def test_solvers_matrix_free(grid, c, s):
    from pysparse_amd import device as dev
    A, S = mf.device_csr(grid, c, s), oracle_for(grid, c, s).A[0]
    solve_with(A, S, grid, dev.DeviceMultigrid32(A, grid), pcg_counts("mf", grid, c, s)[1], "matrix-free %s c %s" % (grid, c))


@pytest.mark.parametrize("galerkin", [False, True])
def test_eigensolvers_reach_the_same_eigenvalues(galerkin):
    from pysparse.eigen import jdsym, lobpcg
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    grid, tol = (20, 24, 28), 1e-8
    A = spmatrix.poisson_csr(*grid)
    K64 = precon.multigrid(A, grid, galerkin=galerkin)
    K32 = precon.multigrid(A, grid, galerkin=galerkin, precision="single")
    assert (K64.precision, K32.precision) == ("double", "single") and K32.galerkin is galerkin
    lam = {}
    for name, K in (("double", K64), ("single", K32)):
        l_lob, _, res, it = lobpcg.lobpcg(A, None, K, 2, tol, 200)
        assert np.all(res <= tol)
        kconv, l_jd, _, it_jd = jdsym.jdsym(A, None, K, 1, 0.0, tol, 300, krylov.qmrs)[:4]
        assert kconv == 1
        lam[name] = (np.asarray(l_lob), np.asarray(l_jd)[:1])
        print("%s galerkin %s: lobpcg %s in %d iterations, jdsym %s in %d" % (name, galerkin, l_lob, it, l_jd[:1], it_jd))
    assert np.abs(lam["single"][0] - lam["double"][0]).max() <= tol
    assert np.abs(lam["single"][1] - lam["double"][1]).max() <= tol
    assert abs(lam["single"][1][0] - lam["single"][0][0]) <= tol  # and both solvers found the same smallest pair


# ------------------------------------------------------------------------------------------------ drop-in

@pytest.mark.parametrize("galerkin", [False, True])
def test_drop_in_module(galerkin):
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    grid = (37, 50)
    A = spmatrix.poisson_csr(*grid)
    K = precon.multigrid(A, grid, galerkin=galerkin, precision="single")
    assert K.precision == "single" and precon.multigrid(A, grid, galerkin=galerkin).precision == "double"
    assert precon.multigrid(A, grid, precision="double").precision == "double"
    assert K.levels == tuple(level_grids(grid)) and K.shape == (1850, 1850)
    with pytest.raises(AttributeError):
        K.precision = "double"
    b = rhs(grid, 11)
    x = np.zeros(b.size)
    info, it, relres = krylov.pcg(A, b, x, 1e-8, 100, K)
    O = oracle_for(grid)
    # the float32 leg of the mode: stored level operators are the Galerkin products of the Poisson operator, not c_a / 4
    leg = Single(GalerkinOracle(grid, O.A[0])) if galerkin else single_mf(grid)
    it32 = numpy_pcg(O.A[0], b, 1e-8, 200, leg.apply)[1]
    print("drop-in pcg galerkin %s: %d iterations (float32 leg: %d)" % (galerkin, it, it32))
    assert info == 0 and abs(it - it32) <= 1
    assert np.linalg.norm(b - O.A[0] @ x) <= 2e-8 * np.linalg.norm(b)
    # the block method of the drop-in object: the single application's bits
    X = np.asfortranarray(np.random.default_rng(4).standard_normal((b.size, 3)))
    Y = np.empty_like(X)
    K.precon_block(X, Y)
    z = np.empty(b.size)
    for c in range(3):
        K.precon(np.ascontiguousarray(X[:, c]), z)
        assert np.array_equal(Y[:, c], z)
