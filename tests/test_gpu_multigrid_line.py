"""GPU: precon.multigrid(..., galerkin=True, line=a) / device.DeviceMultigridLine (psp_mg.hip, psp_mg_line.h; DESIGN.md
section 9h) against the oracle of tests/test_multigrid_line_host.py.

The grids are the smallest that reach each way to go wrong: 3 -> 1 and 2 -> 1 coarsening (5, 6, 9), (7, 12); a single level,
where the handle is the exact inverse (1, 40); many short lines (300, 3) and three long ones (3, 2100); every line axis of
one 3-D grid with odd lengths (33, 17, 65), line 0 being the strided form of the kernel; 4 900 lines, more than one
workgroup and no multiple of 64 (70, 70, 5).  The largest has 36 465 points.

Bounds.  A level operator entry: section 9d's 2 * 3^(2 ND) eps (R |A| P)[K, J].  One application: section 9d's
max(64 eps, 8 e64) max|z_ext| with z_ext the cycle in np.longdouble and e64 the float64 oracle's own distance from it (on
the long lines e64 itself is 1e3 to 1e4 eps: the Thomas solves are as well conditioned as their line operators).

Measured on the MI355X: the worst ratio of an application's error to its bound is 0.84 ((33, 17, 65), line 0, uniform: 54 eps
against the 64 eps floor), 0.69 on (70, 70, 5) graded, at most 0.58 elsewhere; the worst level-operator entry 6.2 eps
(DESIGN.md section 9h)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _p1, numpy_pcg
from test_multigrid_line_host import (EPS, GRADED, LD, LineOracle, graded_operator, line_level_grids, line_oracle_for,
                                      line_oracle_kappa, pcg_counts, rhs)
from test_gpu_multigrid_galerkin import assemble, device_csr_from, device_sss_from, ll_from

pytestmark = pytest.mark.gpu

CASES = [((5, 6, 9), 2), ((7, 12), 1), ((1, 40), 1), ((300, 3), 1), ((3, 2100), 1), ((33, 17, 65), 0), ((33, 17, 65), 1),
         ((33, 17, 65), 2), ((70, 70, 5), 2)]
KAPPA = [((9, 8, 7), 1, "rand1e4"), ((37, 50), 0, "smooth")]  # cell-varying kappa, the Galerkin tests' generator


def cid(c):
    return "x".join(map(str, c[0])) + "-line%d" % c[1]


@functools.lru_cache(maxsize=None)
def device_csr(grid, line, ratio):
    return device_csr_from(line_oracle_for(grid, line, ratio).A[0])


def line_handle(A, grid, line, omega=0.8, steps=2):
    from pysparse_amd import device as dev
    return dev.DeviceMultigridLine(A, grid, omega, steps, line=line)


def test_the_grids_reach_what_they_are_chosen_for():
    assert line_level_grids((5, 6, 9), 2) == [(5, 6, 9), (2, 3, 9), (1, 1, 9)]
    assert line_level_grids((7, 12), 1)[1:] == [(3, 12), (1, 12)] and len(line_level_grids((1, 40), 1)) == 1
    assert 70 * 70 > 64 and (70 * 70) % 64 != 0
    assert max(int(np.prod(g)) for g, _ in CASES) == 36465


# ------------------------------------------------------------------------------------------------ structure

@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("grid,line", CASES, ids=map(cid, CASES))
def test_level_structure(grid, line, steps):
    K = line_handle(device_csr(grid, line, 1.0e4), grid, line, 0.8, steps)
    lv = line_level_grids(grid, line)
    info = K.info()
    assert K.levels == tuple(lv) and info["levels"] == len(lv)
    assert info["dims"] == tuple(tuple(g) + (1,) * (3 - len(g)) for g in lv)
    # section 9h: no tail launch; per level above the last 2 steps sweeps, the restriction and the prolongation, one solve
    assert info["tail_first_level"] == len(lv)
    assert info["launches_per_apply"] == (len(lv) - 1) * (2 * steps + 2) + 1
    assert info["line"] == line and info["galerkin"] is True and info["precision"] == "double"
    assert K.bytes()["operator"] > 0
    K.close()


def test_other_handles_have_no_line_and_the_c_calls_refuse():
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    grid = (5, 6, 9)
    A = device_csr(grid, 2, 1.0e4)
    assert dev.DeviceMultigrid(A, grid, galerkin=True).info()["line"] is None
    assert dev.DeviceMultigrid(dev.DeviceCSR.poisson(5, 6, 9), grid).info()["line"] is None
    assert dev.DeviceMultigridLine(A, grid).info()["line"] is None  # line=None is the point smoother
    g3, g1, g2 = (C.c_int * 3)(5, 6, 9), (C.c_int * 1)(270), (C.c_int * 2)(270, 1)
    for nd, g, axis, why in ((3, g3, 3, b"axes"), (3, g3, -1, b"axes"), (1, g1, 0, b"one axis"), (2, g2, 1, b"at least 2")):
        h = C.c_void_p()
        assert lib().psp_mg_create_csr_line(A._h, nd, g, 0.8, 2, axis, C.byref(h)) == -1 and not h.value
        assert why in lib().psp_last_error(), lib().psp_last_error()


# ------------------------------------------------------------------------------------------------ level operators

@pytest.mark.parametrize("grid,line", CASES, ids=map(cid, CASES))
def test_level_operators(grid, line):
    nd = len(grid)
    S = line_oracle_for(grid, line, 1.0e4).A[0]
    K = line_handle(device_csr(grid, line, 1.0e4), grid, line)
    lv = line_level_grids(grid, line)
    assert K.levels == tuple(lv)
    offs, vals = K.level_operator(0)
    prev = assemble(grid, offs, vals)
    D = (prev - S).tocsr()
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0, "level 0 is not A bit for bit"
    assert np.array_equal(prev.diagonal(), S.diagonal())
    worst = 0.0
    for l in range(1, len(lv)):
        g = lv[l - 1]
        co = [a != line and m >= 2 for a, m in enumerate(g)]
        P = _kron_axes([_p1(m) if c else sp.identity(m, format="csr") for m, c in zip(g, co)]).tocsr()
        R = (P.T / 2.0 ** sum(co)).tocsr()
        offs, vals = K.level_operator(l)
        cur = assemble(lv[l], offs, vals)
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
    print("grid %s line %d: worst level-operator entry error %.2f eps (R|A|P), bound %d eps" % (grid, line, worst, 2 * 3 ** (2 * nd)))
    K.close()


# ------------------------------------------------------------------------------------------------ one application

def check_applications(O, A, grid, line, tag):
    worst = 0.0
    b = np.random.default_rng(3).standard_normal(int(np.prod(grid)))
    for omega in (0.8, 1.0):
        for steps in (1, 2):
            K = line_handle(A, grid, line, omega, steps)
            z = np.full(b.size, np.nan)
            K.precon(b, z)
            K.close()
            zx = O.apply_ext(b, omega, steps)
            scale = float(np.abs(zx).max())
            e64 = float(np.abs(O.apply(b, omega, steps) - zx).max()) / scale
            err = float(np.abs(z - zx).max()) / scale
            bound = max(64.0 * EPS, 8.0 * e64)
            worst = max(worst, err / bound)
            print("%s omega %.1f steps %d: max|z - z_ext| = %.2f eps max|z_ext| (float64 oracle %.2f eps, bound %.1f eps, ratio %.3f)"
                  % (tag, omega, steps, err / EPS, e64 / EPS, bound / EPS, err / bound))
            assert np.isfinite(z).all() and err <= bound, (tag, omega, steps, err / EPS, bound / EPS)
    print("%s: worst ratio to the bound %.3f" % (tag, worst))


@pytest.mark.parametrize("ratio", [1.0, 1.0e4])
@pytest.mark.parametrize("grid,line", CASES, ids=map(cid, CASES))
def test_one_application_against_the_oracle(grid, line, ratio):
    check_applications(line_oracle_for(grid, line, ratio), device_csr(grid, line, ratio), grid, line,
                       "grid %s line %d ratio %g" % (grid, line, ratio))


@pytest.mark.parametrize("grid,line,kind", KAPPA)
def test_one_application_with_varying_kappa(grid, line, kind):
    O = line_oracle_kappa(grid, line, kind)
    check_applications(O, device_csr_from(O.A[0]), grid, line, "grid %s line %d kappa %s" % (grid, line, kind))


def test_a_single_level_is_the_exact_inverse():
    """(1, 40): K(A x) = x to the bound of the extended leg"""
    grid, line = (1, 40), 1
    O = line_oracle_for(grid, line, 1.0e4)
    x = np.random.default_rng(5).standard_normal(40)
    b = O.A[0] @ x
    z = np.empty(40)
    line_handle(device_csr(grid, line, 1.0e4), grid, line).precon(b, z)
    zx = O.apply_ext(b)
    scale = float(np.abs(zx).max())
    e64 = float(np.abs(O.apply(b) - zx).max()) / scale
    assert np.abs(z - zx).max() <= max(64.0 * EPS, 8.0 * e64) * scale
    assert np.abs(z - x).max() <= 1e-9 * np.abs(x).max()  # and that is x itself, up to the conditioning of the line


# ------------------------------------------------------------------------------------------------ same bits

@pytest.mark.parametrize("grid,line", CASES, ids=map(cid, CASES))
def test_same_bits(grid, line):
    from pysparse_amd import device as dev
    S = line_oracle_for(grid, line, 1.0e4).A[0]
    K = line_handle(device_csr(grid, line, 1.0e4), grid, line)
    n = S.shape[0]
    b = np.random.default_rng(7).standard_normal(n)
    z1, z2 = np.empty(n), np.empty(n)
    K.precon(b, z1)
    K.precon(b, z2)
    assert np.array_equal(z1, z2)
    xb, yb = dev.DeviceBuffer.from_host(b), dev.DeviceBuffer(n)
    yb.zero()
    K.precon_dev(xb.ptr, yb.ptr)
    assert np.array_equal(yb.download(), z1)
    assert np.array_equal(xb.download(), b)  # x is unchanged
    # an sss_mat handle of the same matrix
    Ks = line_handle(device_sss_from(S), grid, line)
    assert Ks.info()["line"] == line
    z3 = np.empty(n)
    Ks.precon(b, z3)
    assert np.array_equal(z3, z1)
    for l in range(len(K.levels)):
        assert np.array_equal(K.level_operator(l)[1], Ks.level_operator(l)[1])
    # column c of a block is the single cycle on column c; a line handle keeps no block vectors
    B = np.asfortranarray(np.random.default_rng(8).standard_normal((n, 3)))
    B[:, 1] = b
    Y = np.full((n, 3), np.nan, order="F")
    K.precon_block(B, Y)
    assert np.array_equal(Y[:, 1], z1)
    for c in (0, 2):
        zc = np.empty(n)
        K.precon(np.ascontiguousarray(B[:, c]), zc)
        assert np.array_equal(Y[:, c], zc)
    assert K.block_info() == {"columns": 0, "bytes": 0}


# ------------------------------------------------------------------------------------------------ refusal at creation

def test_a_failing_line_pivot_is_singular():
    """a symmetric 5-point operator with a positive diagonal -- galerkin=True's checks let it through -- whose couplings
    along the line axis are three times what the diagonal carries: p_1 = d_1 - l_1^2 / d_0 < 0"""
    from pysparse_amd import device as dev
    grid, line = (5, 6), 1
    S = graded_operator(grid, line, 10.0)
    Cc = S.tocoo()
    along = np.abs(Cc.row - Cc.col) == 5
    bad = sp.coo_matrix((np.where(along, 3.0 * Cc.data, Cc.data), (Cc.row, Cc.col)), shape=S.shape).tocsr()
    bad.sort_indices()
    assert abs(bad - bad.T).max() == 0.0 and bad.diagonal().min() > 0.0
    A = device_csr_from(bad)
    from pysparse_amd._capi import PspError, lib
    with pytest.raises(PspError, match="pivot"):
        line_handle(A, grid, line)
    h = C.c_void_p()
    g = (C.c_int * 2)(*grid)
    assert lib().psp_mg_create_csr_line(A._h, 2, g, 0.8, 2, line, C.byref(h)) == -4 and not h.value  # PSP_ESINGULAR
    line_handle(device_csr_from(S), grid, line).close()  # the operator itself is accepted


# ------------------------------------------------------------------------------------------------ solvers

@pytest.mark.parametrize("grid,line,ratio", GRADED, ids=[cid(c) for c in GRADED])
def test_pcg_on_the_graded_grids(grid, line, ratio):
    """the count of the oracle-preconditioned NumPy PCG within one, the true residual, and at most a third of the
    point-smoothed Galerkin handle's count on the same operator"""
    from pysparse_amd import device as dev
    O = line_oracle_for(grid, line, ratio)
    S, A = O.A[0], device_csr(grid, line, ratio)
    b = rhs(S.shape[0])
    _, want = pcg_counts(grid, line, ratio, point=False)
    x = np.zeros(b.size)
    info, it, relres = dev.pcg(A, b, x, 1e-8, 500, line_handle(A, grid, line))
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    xp = np.zeros(b.size)
    infop, itp, _ = dev.pcg(A, b, xp, 1e-8, 500, dev.DeviceMultigrid(A, grid, galerkin=True))
    print("pcg %s line %d ratio %g: info %d, %d iterations (oracle %d), true residual %.3e; point-smoothed handle %d iterations"
          % (grid, line, ratio, info, it, want, res, itp))
    assert info == 0 and abs(it - want) <= 1
    assert res <= 1e-8
    assert infop == 0 and 3 * it <= itp


@pytest.mark.parametrize("grid,line,ratio", [((5, 6, 9), 2, 1.0), ((70, 70, 5), 2, 1.0e4), ((33, 17, 65), 0, 1.0e4)])
def test_pcg_counts_on_other_grids(grid, line, ratio):
    from pysparse_amd import device as dev
    S, A = line_oracle_for(grid, line, ratio).A[0], device_csr(grid, line, ratio)
    b = rhs(S.shape[0])
    _, want = pcg_counts(grid, line, ratio, point=False)
    x = np.zeros(b.size)
    info, it, _ = dev.pcg(A, b, x, 1e-8, 500, line_handle(A, grid, line))
    assert info == 0 and abs(it - want) <= 1
    assert np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b)


def test_minres_and_pcg_batch_take_the_handle():
    from pysparse_amd import device as dev
    grid, line, ratio = (24, 40, 20), 1, 1.0e3
    S, A = line_oracle_for(grid, line, ratio).A[0], device_csr(grid, line, ratio)
    n = S.shape[0]
    K = line_handle(A, grid, line)
    b = rhs(n)
    x = np.zeros(n)
    info, it, _ = dev.minres(A, b, x, 1e-8, 200, K)
    assert info == 0 and it <= 20 and np.linalg.norm(b - S @ x) <= 1e-7 * np.linalg.norm(b)
    B = np.asfortranarray(np.random.default_rng(2).random((n, 3)))
    X = np.zeros((n, 3), order="F")
    info, it, relres = dev.pcg_batch(A, B, X, 1e-8, 200, K)
    for c in range(3):
        xs = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), xs, 1e-8, 200, K)
        assert info[c] == 0 and (info[c], it[c]) == r[:2] and np.array_equal(X[:, c], xs)
        assert np.linalg.norm(B[:, c] - S @ X[:, c]) <= 1e-8 * np.linalg.norm(B[:, c])


def test_lobpcg_and_the_drop_in_module_take_the_handle():
    from pysparse.eigen import lobpcg
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    grid, line = (20, 24), 1
    S = graded_operator(grid, line, 1.0e3)
    A = ll_from(S).to_csr()
    K = precon.multigrid(A, grid, galerkin=True, line=line)
    assert K.line == line and K.galerkin is True and K.levels == tuple(line_level_grids(grid, line))
    assert precon.multigrid(A, grid, galerkin=True).line is None
    lam, Q, res, it = lobpcg.lobpcg(A, None, K, 2, 1e-8, 300)
    spec = np.linalg.eigvalsh(S.toarray())
    assert res.max() <= 1e-8 and np.abs(lam - spec[:2]).max() <= 1e-7 * spec[1]
    b = rhs(S.shape[0])
    x = np.zeros(b.size)
    info, it, _ = krylov.pcg(A, b, x, 1e-8, 100, K)
    assert info == 0 and it <= 15 and np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b)
