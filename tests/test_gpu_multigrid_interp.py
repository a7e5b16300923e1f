"""GPU: precon.multigrid(..., galerkin=True, interp='operator') / device.DeviceMultigridInterp (psp_mg.hip, psp_mg_interp.h;
DESIGN.md section 9j) against the oracle and the operators of tests/test_multigrid_interp_host.py.

The cases are GPU_CASES of the host file: (7,) a single transfer onto three points, (64,) five; (9, 7) and (13, 11) odd
lengths, where the last point of an axis has no upper parent; (40, 5) an axis that stops coarsening after one level;
(70, 45) and (64, 64) more than one restriction tile; (6, 7, 9), (9, 7, 6), (8, 8, 8) three axes with even and odd lengths;
(26, 37, 21) and (32, 32, 32) several tiles along every axis and three transfers.  kappa comes in blocks of 1e4 or 1e6, once
smooth and once constant with a shift; three cases are 9- / 27-point operators for stencil='box'.  Every one satisfies the
decision margin that the host file asserts, so the device and the oracle take the same branch at every point.

Bounds.
  A weight: the oracle's weights are formed from the DOWNLOADED level operator with the kernel's order of the collapse, so
  both sides start from the same T.  Each side then rounds, per term, one quotient and one product, and adds at most 26
  terms: either is within (26 + 2) eps sum |T/T0| |w| of the exact sum, the two within c = 56 times that, accumulated
  through the rounds by the host file's E.  Fallback counts per level are the oracle's, exactly.
  A level operator entry, against SciPy's R A P with P from the downloaded weights: section 9d's rule with the new term
  count.  An entry sums at most 3^(2 ND) terms a * ((w_i w_j) 2^-k), two roundings each where the linear weights had none,
  allowed on either side: 2 (3^(2 ND) + 2) eps (|R| |A| |P|)[K, J].  (The kernel rounds an entry once; SciPy's products do
  not.  Measured: at most 1.93 eps.)
  One application: section 9d's max(64 eps, 8 e64) max|z_ext|.
  PCG takes exactly the iterations of the host file's table with a true residual <= 1e-8 ||b||, but for the three rows the
  host file lists as UNSTABLE (blocks of 1e6 at 64^2, 128^2 and (26, 37, 21): cond * eps = the tolerance), where the oracle's
  own solve gives other counts when its cycle is evaluated in np.longdouble or its dot products are summed in another
  order, or misses that residual; there a count inside the range of the oracle's variations and a true residual of at most
  twice the worst of theirs are asserted (the host file records and checks both).
  Measured on the MI355X: 20 iterations at 64^2 (oracle 19 - 20, true residual 1.25e-8), 54 at 128^2 (oracle 52 - 59, true
  residual 1.15e-7), 33 at (26, 37, 21) (oracle 33 - 34, true residual 6.3e-9).  The count of the linear handle is printed
  beside the table's, not asserted: on the single-cell operator it is 194 where NumPy PCG with section 9d's oracle takes 197.

The case nearest to section 9d's bound of one application is (70, 45) with blocks of 1e6: 139 084 - 164 639 eps max|z_ext|
where the float64 oracle is at 22 162 - 25 637 eps, ratios to the bound 0.825, 0.790, 0.776, 0.815.  Level 3 of that operator
(8 x 5 points, one of them a fallback point) is 30 eps from the np.longdouble chain in the float64 oracle, and the two level
operators below it, formed with the weights derived from it, are 2e5 eps away: the collapse T0 cancels and the weights
amplify the rounding errors of the operator they are formed from, in the oracle's float64 leg too.  With level operators
whose products were rounded before they were summed (1.6 eps per entry) the device stood at 1.038, 0.995, 0.977, 1.026 of the
bound and missed it; mg_galerkin_w_kernel now sums the exact products and rounds once."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import level_grids
from test_multigrid_interp_host import (GPU_CASES, OP_SEED, PCG_TABLE, UNSTABLE, interp_operator, interp_oracle_for,
                                        operator_weights, prolongation, rhs)
import test_gpu_multigrid_galerkin as gk

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_WEIGHT = 56.0
gid = gk.gid
CASES = [pytest.param(g, k, s, sd, id="%s-%s" % (gid(g), k)) for g, k, s, sd in GPU_CASES]


@functools.lru_cache(maxsize=None)
def device_csr(grid, kind, s=0.0, seed=0):
    return gk.device_csr_from(interp_operator(grid, kind, s, seed))


def handle(A, grid, kind, omega=0.8, steps=2, **kw):
    from pysparse_amd import device as dev
    return dev.DeviceMultigridInterp(A, grid, omega, steps, stencil="box" if kind.startswith("box_") else "axis", **kw)


def triples(M):
    C = sp.coo_matrix(M)
    keep = C.data != 0.0
    return C.row[keep], C.col[keep], C.data[keep]


# ------------------------------------------------------------------------------------------------ structure

@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("grid,kind", [((7,), "b2_1e4"), ((3,), "const"), ((40, 5), "b4_1e4"), ((13, 11), "box_b3_1e6"),
                                       ((9, 7, 6), "b3_1e6")], ids=lambda v: gid(v) if isinstance(v, tuple) else v)
def test_structure(grid, kind, steps):
    from pysparse_amd import device as dev
    A = device_csr(grid, kind)
    K = handle(A, grid, kind, 0.8, steps)
    lv = level_grids(grid)
    info = K.info()
    assert K.levels == tuple(lv) and info["levels"] == len(lv)
    # no tail launch: every level above the last is launches, the dense product of the last one is one more
    assert info["tail_first_level"] == len(lv)
    assert info["launches_per_apply"] == (len(lv) - 1) * (max(steps - 1, 1) + steps + 2) + 1
    assert info["galerkin"] is True and info["line"] is None and info["precision"] == "double"
    assert K.interp == "operator"
    with pytest.raises(AttributeError):
        K.interp = "linear"
    # the weights count as operator bytes: 2^nd arrays per level above the last
    L = dev.DeviceMultigridInterp(A, grid, 0.8, steps, stencil=K.stencil, interp="linear")
    assert L.interp == "linear"
    weights = sum(8 * 2 ** len(grid) * int(np.prod(g)) for g in lv[:-1])
    assert weights - 16384 < K.bytes()["operator"] - L.bytes()["operator"] <= weights  # (the linear handle has the tail's table)
    for l in range(len(lv) - 1):
        assert K.transfer_weights(l).shape == (2 ** len(grid), int(np.prod(lv[l])))
    with pytest.raises(ValueError, match="no transfer"):
        K.transfer_weights(len(lv) - 1)
    with pytest.raises(ValueError, match="interp='linear'"):
        L.transfer_weights(0)
    with pytest.raises(ValueError, match="interp='linear'"):
        L.interp_fallbacks(0)
    # the block entry points run the single cycle column by column: no block vectors
    n = int(np.prod(grid))
    X = np.asfortranarray(np.random.default_rng(1).standard_normal((n, 2)))
    K.precon_block(X, np.empty((n, 2), order="F"))
    K.block_reserve(4)
    assert K.block_info() == {"columns": 0, "bytes": 0}


# ------------------------------------------------------------------------------------------------ weights and level operators

@pytest.mark.parametrize("grid,kind,s,seed", CASES)
def test_weights_and_level_operators(grid, kind, s, seed):
    nd = len(grid)
    O = interp_oracle_for(grid, kind, s, seed)
    K = handle(device_csr(grid, kind, s, seed), grid, kind)
    lv = level_grids(grid)
    offs, vals = K.level_operator(0)
    prev = gk.assemble(grid, offs, vals)
    D = (prev - O.A[0]).tocsr()
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0, "level 0 is not A bit for bit"
    worst_w = worst_a = 0.0
    for l in range(len(lv) - 1):
        g = lv[l]
        # the weights, from the level operator the device holds
        W = K.transfer_weights(l)
        Wo, fb, margin, E = operator_weights(g, *triples(prev), c_eps=C_WEIGHT * EPS)
        assert margin > 1e-9
        assert K.interp_fallbacks(l) == O.fallbacks[l] == fb, (grid, kind, l)
        err = np.abs(W - Wo)
        assert np.isfinite(W).all() and (err <= E).all(), (grid, kind, l, float((err - E).max()))
        nz = E > 0
        if nz.any():
            worst_w = max(worst_w, float((err[nz] / E[nz]).max()))
        # the next level operator, from the weights the device holds
        r, c, v, shape = prolongation(g, W)
        P = sp.csr_matrix((v, (r, c)), shape=shape)
        scale = 1.0 / 2.0 ** sum(m >= 4 for m in g)
        R = (P.T * scale).tocsr()
        offs, vals = K.level_operator(l + 1)
        cur = gk.assemble(lv[l + 1], offs, vals)
        refs = (R @ prev @ P).tocsr()
        mag = (abs(R) @ abs(prev) @ abs(P)).tocsr()
        bound = 2.0 * (3 ** (2 * nd) + 2) * EPS * mag
        errA = abs(cur - refs).tocsr()
        over = (errA - bound).tocsr()
        assert over.nnz == 0 or over.data.max() <= 0.0, (grid, kind, l + 1, over.data.max())
        inv = mag.copy()
        inv.eliminate_zeros()
        inv.data = 1.0 / inv.data
        worst_a = max(worst_a, errA.multiply(inv).max() / EPS)
        prev = cur
    print("grid %s %s: worst weight error %.3f of its bound (c = %d), fallbacks %s; worst level-operator entry error %.2f eps "
          "(|R||A||P|), bound %d eps" % (grid, kind, worst_w, C_WEIGHT, O.fallbacks, worst_a, 2 * (3 ** (2 * nd) + 2)))
    K.close()


# ------------------------------------------------------------------------------------------------ one application

@pytest.mark.parametrize("grid,kind,s,seed", CASES)
def test_one_application_against_the_oracle(grid, kind, s, seed):
    A, O = device_csr(grid, kind, s, seed), interp_oracle_for(grid, kind, s, seed)
    worst, missed = 0.0, []
    for omega in (0.8, 1.0):
        for steps in (1, 2):
            K = handle(A, grid, kind, omega, steps)
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
            assert np.isfinite(z).all()
            if not err <= bound:  # every (omega, steps) is measured before the case fails
                missed.append((omega, steps, err / EPS, bound / EPS))
            K.close()
    print("grid %s %s: worst ratio to the bound %.3f" % (grid, kind, worst))
    assert not missed, (grid, kind, missed)


# ------------------------------------------------------------------------------------------------ same bits

@pytest.mark.parametrize("grid,kind,s,seed", CASES)
def test_same_bits(grid, kind, s, seed):
    from pysparse_amd import device as dev
    S = interp_oracle_for(grid, kind, s, seed).A[0]
    K = handle(device_csr(grid, kind, s, seed), grid, kind)
    n = int(np.prod(grid))
    b = rhs(grid, 3)
    z1, z2 = np.empty(n), np.empty(n)
    K.precon(b, z1)
    K.precon(b, z2)
    assert np.array_equal(z1, z2)
    xb, yb = dev.DeviceBuffer.from_host(b), dev.DeviceBuffer(n)
    yb.zero()
    K.precon_dev(xb.ptr, yb.ptr)
    assert np.array_equal(yb.download(), z1)
    assert np.array_equal(xb.download(), b)  # x is unchanged
    # an sss_mat handle of the same matrix, and a second csr handle built from scratch
    for other in (handle(gk.device_sss_from(S), grid, kind), handle(gk.device_csr_from(S), grid, kind)):
        assert other.interp == "operator"
        z3 = np.empty(n)
        other.precon(b, z3)
        assert np.array_equal(z3, z1)
        for l in range(len(K.levels)):
            assert np.array_equal(K.level_operator(l)[1], other.level_operator(l)[1])
        for l in range(len(K.levels) - 1):
            assert np.array_equal(K.transfer_weights(l), other.transfer_weights(l))
            assert K.interp_fallbacks(l) == other.interp_fallbacks(l)
    # column c of a block, from host blocks and from device blocks with a leading dimension above n
    pad = 5
    for k in (1, 3):
        X = np.asfortranarray(np.random.default_rng(20 + k).random((n, k)))
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
    assert K.block_info()["columns"] == 0


@pytest.mark.parametrize("grid,kind", [((64,), "b5_1e6"), ((70, 45), "b5_1e6"), ((9, 7, 6), "b3_1e6"), ((13, 11), "box_b3_1e6")],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else v)
def test_the_default_is_unchanged(grid, kind):
    """interp='linear' is the handle made without the keyword: the same info, level operators, bytes and bits, through
    device.py and through the drop-in module"""
    from pysparse.precon import precon
    from pysparse_amd import device as dev
    S = interp_oracle_for(grid, kind).A[0]
    A = device_csr(grid, kind)
    box = kind.startswith("box_")
    K0 = dev.DeviceMultigridBox(A, grid) if box else dev.DeviceMultigrid(A, grid, galerkin=True)
    K1 = dev.DeviceMultigridInterp(A, grid, stencil="box" if box else "axis", interp="linear")
    assert K0.info() == K1.info() and K0.bytes() == K1.bytes() and K0.interp == K1.interp == "linear"
    b = rhs(grid, 2)
    z0, z1, z2, z3 = (np.empty(b.size) for _ in range(4))
    K0.precon(b, z0)
    K1.precon(b, z1)
    assert np.array_equal(z0, z1)
    for l in range(len(K0.levels)):
        assert np.array_equal(K0.level_operator(l)[1], K1.level_operator(l)[1])
    kw = {"stencil": "box"} if box else {}
    Al = gk.ll_from(S).to_csr()
    P0 = precon.multigrid(Al, grid, galerkin=True, **kw)
    P1 = precon.multigrid(Al, grid, galerkin=True, interp="linear", **kw)
    assert P0.interp == P1.interp == "linear"
    P0.precon(b, z2)
    P1.precon(b, z3)
    assert np.array_equal(z2, z0) and np.array_equal(z3, z0)


# ------------------------------------------------------------------------------------------------ solves

@pytest.mark.parametrize("kind,grid", sorted(PCG_TABLE), ids=lambda v: v if isinstance(v, str) else gid(v))
def test_pcg_takes_the_iterations_of_the_table(kind, grid):
    from pysparse_amd import device as dev
    seed, want, wantl, wantj = PCG_TABLE[(kind, grid)]
    ops = OP_SEED.get((kind, grid), 0)
    A, S = device_csr(grid, kind, 0.0, ops), interp_operator(grid, kind, 0.0, ops)
    b = rhs(grid, seed)
    K = handle(A, grid, kind)
    x = np.zeros(b.size)
    info, it, relres = dev.pcg(A, b, x, 1e-8, 3000, K)
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    xl = np.zeros(b.size)
    box = kind.startswith("box_")
    Kl = dev.DeviceMultigridBox(A, grid) if box else dev.DeviceMultigrid(A, grid, galerkin=True)
    infol, itl, _ = dev.pcg(A, b, xl, 1e-8, 3000, Kl)
    print("pcg %s %s: info %d, %d iterations (table: %d), true residual %.3e; with linear interpolation %d (table: %d)"
          % (kind, grid, info, it, want, res, itl, wantl))
    assert info == 0 and infol == 0
    if (kind, grid) in UNSTABLE:  # the oracle itself does not pin these rows down (the host file says why)
        lo, hi, worst = UNSTABLE[(kind, grid)]
        print("  an unstable row: the oracle takes %d to %d iterations over its own variations, worst true residual %.2e" % (lo, hi, worst))
        assert lo <= it <= hi and res <= 2.0 * worst and it < itl
        return
    assert it == want and res <= 1e-8


@pytest.mark.parametrize("kind,grid", [("b8_1e4", (64, 64)), ("b3_1e6", (9, 7, 6))], ids=["64x64", "9x7x6"])
def test_pcg_batch_ends_each_column_as_the_single_solve(kind, grid):
    from pysparse_amd import device as dev
    A = device_csr(grid, kind)
    n = int(np.prod(grid))
    K = handle(A, grid, kind)
    B = np.asfortranarray(np.random.default_rng(2).random((n, 3)))
    X = np.zeros((n, 3), order="F")
    info, it, relres = dev.pcg_batch(A, B, X, 1e-8, 200, K)
    for c in range(3):
        x = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-8, 200, K)
        assert r[0] == 0 and (info[c], it[c]) == r[:2] and relres[c] == r[2]
        assert np.array_equal(X[:, c], x)


def test_the_drop_in_module_lobpcg_and_pcg():
    from pysparse.eigen import lobpcg
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    kind, grid = "b8_1e4", (64, 64)
    seed, want, _, _ = PCG_TABLE[(kind, grid)]
    S = interp_operator(grid, kind)
    A = gk.ll_from(S).to_csr()
    K = precon.multigrid(A, grid, galerkin=True, interp="operator")
    assert K.interp == "operator" and K.galerkin is True and K.line is None and K.stencil == "axis"
    assert K.levels == tuple(level_grids(grid))
    with pytest.raises(AttributeError):
        K.interp = "linear"
    b = rhs(grid, seed)
    x = np.zeros(b.size)
    info, it, relres = krylov.pcg(A, b, x, 1e-8, 200, K)
    assert info == 0 and it == want and np.linalg.norm(b - S @ x) <= 1e-8 * np.linalg.norm(b)
    lam, Q, res, its = lobpcg.lobpcg(A, None, K, 3, 1e-8, 300)
    print("lobpcg k = 3 on %s %s: %d iterations, eigenvalues %s, residuals %s" % (kind, grid, its, lam, res))
    assert np.all(np.asarray(res) <= 1e-8)
    R = S @ Q - Q * np.asarray(lam)
    assert np.linalg.norm(R, axis=0).max() <= 1e-6 * abs(S).max()


# ------------------------------------------------------------------------------------------------ refusals

def test_device_side_refusals_reach_the_caller_unchanged():
    from pysparse_amd import device as dev

    def refused(M, grid, why, stencil="axis"):
        with pytest.raises(ValueError, match=why) as e:
            dev.DeviceMultigridInterp(gk.device_csr_from(M), grid, stencil=stencil)
        with pytest.raises(ValueError) as e0:  # the text of the handle without the keyword
            (dev.DeviceMultigridBox if stencil == "box" else dev.DeviceMultigrid)(gk.device_csr_from(M), grid, galerkin=True)
        assert str(e.value) == str(e0.value)

    grid = (9, 7)
    S = interp_operator(grid, "b2_1e4")
    dev.DeviceMultigridInterp(gk.device_csr_from(S), grid).close()  # the unchanged matrix is accepted
    P = S.tolil()
    P[20, 22] = P[22, 20] = -1.0  # two points away along axis 0
    refused(P.tocsr(), grid, "no axis stride")
    refused(P.tocsr(), grid, "offset", stencil="box")
    P = S.tolil()
    P[8, 9] = P[9, 8] = -1.0  # across a line end
    refused(P.tocsr(), grid, "wraps")
    P = S.copy()
    k = P.indptr[20] + list(P.indices[P.indptr[20]:P.indptr[21]]).index(21)
    P.data[k] = np.nextafter(P.data[k], 0.0)
    refused(P, grid, "unsymmetric")
    P = S.copy()
    k = P.indptr[20] + list(P.indices[P.indptr[20]:P.indptr[21]]).index(20)
    P.data[k] = -1.0
    refused(P, grid, "diagonal")
    # the 9-point operator without stencil='box'
    refused(interp_operator((13, 11), "box_b3_1e6"), (13, 11), "no axis stride")
    g3 = (9, 8, 7)
    rel = dev.DeviceCSR.poisson(*g3)
    rel.release_arrays()
    with pytest.raises(ValueError, match="index arrays"):
        dev.DeviceMultigridInterp(rel, g3)
    with pytest.raises(ValueError):
        dev.DeviceMultigridInterp(dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0]), (9, 8))
    # the C ABI: the bit needs the Galerkin bit and does not go with the single-precision bit
    import ctypes as C
    from pysparse_amd import _capi
    h, g = C.c_void_p(), (C.c_int * 2)(9, 7)
    A = gk.device_csr_from(S)
    for flags, word in ((dev.PSP_MG_INTERP, b"PSP_MG_GALERKIN"), (dev.PSP_MG_INTERP | dev.PSP_MG_BOX, b"PSP_MG_GALERKIN"),
                        (dev.PSP_MG_INTERP | dev.PSP_MG_GALERKIN | dev.PSP_MG_SINGLE, b"not supported")):
        assert _capi.lib().psp_mg_create_csr_ex(A._h, 2, g, 0.8, 2, flags, C.byref(h)) == -1 and h.value is None
        assert word in _capi.lib().psp_last_error()
