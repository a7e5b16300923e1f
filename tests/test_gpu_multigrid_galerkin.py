"""GPU: precon.multigrid(..., galerkin=True) / device.DeviceMultigrid(..., galerkin=True) (psp_mg.hip, psp_mg_galerkin.h;
DESIGN.md section 9d) against the oracle of tests/test_multigrid_galerkin_host.py.

The grids are the smallest that reach each way to go wrong: 1-D with two launch-per-step levels above the tail
(4100,); everything inside the tail; a 9-point level of 2 145 points just above the tail's 2 048 (130, 67); semi-coarsening
(16, 16, 3); a grid that crosses the restriction tile in every axis with odd and even lengths and has a 27-point level of
4 080 points above the tail (33, 31, 35).  The largest has 35 805 points.

Bounds.  A level operator entry: 2 * 3^(2 ND) eps (R |A| P)[K, J] -- the worst case of two summation orders over at most
3^(2 ND) exactly scaled terms (derived, not measured).  One application: max(64 eps, 8 e64) max|z_ext| with z_ext the cycle
in np.longdouble and e64 the float64 SciPy oracle's own distance from it: 64 eps is section 9c's asserted bound, the
factor 8 covers another summation order against a single realisation of the float64 error."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import _kron_axes, _p1, level_grids, numpy_pcg
from test_multigrid_galerkin_host import galerkin_oracle_for, varying_operator, GalerkinOracle

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TAIL_T = 2048  # the largest level the tail launch takes (as in 9c)

GRIDS = [(7,), (64,), (4100,), (5, 4), (37, 50), (130, 67), (9, 8, 7), (16, 16, 3), (20, 24, 28), (33, 31, 35)]


def gid(g):
    return "x".join(map(str, g))


def device_csr_from(S):
    from pysparse_amd import device as dev
    return dev.DeviceCSR.from_arrays(S.shape, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)


def device_sss_from(S):
    from pysparse_amd import device as dev
    L = sp.tril(S, -1, format="csr")
    L.sort_indices()
    return dev.DeviceSSS.from_arrays(S.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data,
                                     S.diagonal().copy())


@functools.lru_cache(maxsize=None)
def device_csr(grid, kind, s):
    return device_csr_from(galerkin_oracle_for(grid, kind, s).A[0])


def rhs(grid, seed=0):
    return np.random.default_rng(seed).standard_normal(int(np.prod(grid)))


def expected_structure(grid, steps):
    lv = level_grids(grid)
    tail_first = next(l for l, g in enumerate(lv) if int(np.prod(g)) <= TAIL_T)
    # section 9d: per level above the tail the pre-smoothing (sweeps one and two are one pass), the restriction, the
    # prolongation and `steps` sweeps; one launch for the tail
    launches = 1 + tail_first * ((steps - 1 if steps >= 2 else 1) + 2 + steps)
    return lv, tail_first, launches


def test_the_grids_reach_what_they_are_chosen_for():
    sizes = lambda g: [int(np.prod(l)) for l in level_grids(g)]  # noqa: E731
    assert sizes((130, 67))[1] == 2145 and sizes((33, 31, 35))[1] == 4080 and sizes((33, 31, 35))[2] <= TAIL_T
    assert sum(n > TAIL_T for n in sizes((4100,))) == 2
    assert max(int(np.prod(g)) for g in GRIDS) == 35805
    assert level_grids((16, 16, 3))[-1] == (2, 2, 3)


# ------------------------------------------------------------------------------------------------ level operators

def assemble(grid, offs, vals):
    """the matrix of a downloaded level: array k holds A[K, K + o_k]; also checks that every entry whose neighbour does not
    exist is exactly 0"""
    g3 = tuple(grid) + (1,) * (3 - len(grid))
    n = int(np.prod(g3))
    k = np.arange(n)
    co = (k % g3[0], (k // g3[0]) % g3[1], k // (g3[0] * g3[1]))
    assert offs[0] == (0, 0, 0)
    rows, cols, data = [k], [k], [vals[0]]
    for a, d in enumerate(offs[1:], 1):
        assert d != (0, 0, 0) and all(abs(x) <= 1 for x in d)
        lin = d[0] + g3[0] * (d[1] + g3[1] * d[2])
        assert d[::-1] < (0, 0, 0), "a lower offset"
        ok = np.ones(n, dtype=bool)
        for c, x, m in zip(co, d, g3):
            ok &= (c + x >= 0) & (c + x < m)
        assert not vals[a][~ok].any(), "an entry outside the grid is not exactly 0"
        rows += [k[ok], k[ok] + lin]
        cols += [k[ok] + lin, k[ok]]
        data += [vals[a][ok], vals[a][ok]]
    return sp.coo_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


@pytest.mark.parametrize("kind", ["smooth", "rand1e4"])
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_level_operators(grid, kind):
    from pysparse_amd import device as dev
    nd = len(grid)
    S = galerkin_oracle_for(grid, kind, 0.3).A[0]
    K = dev.DeviceMultigrid(device_csr(grid, kind, 0.3), grid, galerkin=True)
    lv = level_grids(grid)
    assert K.levels == tuple(lv)
    offs, vals = K.level_operator(0)
    assert list(offs[1:]) == [tuple(-int(a == b) for b in range(3)) for a in range(nd)]
    prev = assemble(grid, offs, vals)
    D = (prev - S).tocsr()
    assert D.nnz == 0 or np.abs(D.data).max() == 0.0, "level 0 is not A bit for bit"
    assert np.array_equal(prev.diagonal(), S.diagonal())
    worst = 0.0
    for l in range(1, len(lv)):
        g = lv[l - 1]
        co = [m >= 4 for m in g]
        P = _kron_axes([_p1(m) if c else sp.identity(m, format="csr") for m, c in zip(g, co)]).tocsr()
        R = (P.T / 2.0 ** sum(co)).tocsr()
        offs, vals = K.level_operator(l)
        assert len(offs) == 1 + (3 ** nd - 1) // 2 and len(set(offs)) == len(offs)
        cur = assemble(lv[l], offs, vals)
        refs = (R @ prev @ P).tocsr()
        mag = (R @ abs(prev) @ P).tocsr()
        # every entry of the reference lies inside the pattern that is stored: nothing is lost
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

@pytest.mark.parametrize("s", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["smooth", "rand1e4"])
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_one_application_against_the_oracle(grid, kind, s):
    from pysparse_amd import device as dev
    A, O = device_csr(grid, kind, s), galerkin_oracle_for(grid, kind, s)
    worst = 0.0
    for omega, steps in ((0.8, 2), (1.0, 1), (2.0 / 3.0, 3)):
        K = dev.DeviceMultigrid(A, grid, omega, steps, galerkin=True)
        for seed in (0, 1):
            b = rhs(grid, seed)
            z = np.full(b.size, np.nan)
            K.precon(b, z)
            zx = O.apply_ext(b, omega, steps)
            scale = float(np.abs(zx).max())
            e64 = float(np.abs(O.apply(b, omega, steps) - zx).max()) / scale
            err = float(np.abs(z - zx).max()) / scale
            bound = max(64.0 * EPS, 8.0 * e64)
            worst = max(worst, err / bound)
            print("grid %s %s s %.1f omega %.4f steps %d seed %d: max|z - z_ext| = %.2f eps max|z_ext| (float64 oracle %.2f eps, "
                  "bound %.1f eps, ratio %.3f)" % (grid, kind, s, omega, steps, seed, err / EPS, e64 / EPS, bound / EPS, err / bound))
            assert np.isfinite(z).all() and err <= bound, (grid, kind, s, omega, steps, err / EPS, bound / EPS)
        K.close()
    print("grid %s %s s %.1f: worst ratio to the bound %.3f" % (grid, kind, s, worst))


# ------------------------------------------------------------------------------------------------ same bits

@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_same_bits(grid):
    from pysparse_amd import device as dev
    S = galerkin_oracle_for(grid, "rand1e4", 0.3).A[0]
    K = dev.DeviceMultigrid(device_csr(grid, "rand1e4", 0.3), grid, galerkin=True)
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
    # an sss_mat handle of the same matrix
    Ks = dev.DeviceMultigrid(device_sss_from(S), grid, galerkin=True)
    assert Ks.info()["galerkin"] is True
    z3 = np.empty(b.size)
    Ks.precon(b, z3)
    assert np.array_equal(z3, z1)
    # a second handle built from scratch: the level operators are the same bits too
    K2 = dev.DeviceMultigrid(device_csr_from(S), grid, galerkin=True)
    for l in range(len(K.levels)):
        assert np.array_equal(K.level_operator(l)[1], K2.level_operator(l)[1])
        assert np.array_equal(K.level_operator(l)[1], Ks.level_operator(l)[1])


# ------------------------------------------------------------------------------------------------ accept and refuse

def check_application(S, grid, K, tag):
    O = GalerkinOracle(grid, S)
    b = rhs(grid, 5)
    z = np.full(b.size, np.nan)
    K.precon(b, z)
    zx = O.apply_ext(b)
    scale = float(np.abs(zx).max())
    e64 = float(np.abs(O.apply(b) - zx).max()) / scale
    err = float(np.abs(z - zx).max()) / scale
    print("%s: %.2f eps (float64 oracle %.2f eps)" % (tag, err / EPS, e64 / EPS))
    assert err <= max(64.0 * EPS, 8.0 * e64)


def test_accepted_operators():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    # the constant-coefficient operator is one of the accepted ones
    S = varying_operator(grid, "const", 0.0)
    K = dev.DeviceMultigrid(device_csr_from(S), grid, galerkin=True)
    assert K.info()["galerkin"] is True and dev.DeviceMultigrid(device_csr_from(S), grid).info()["galerkin"] is False
    check_application(S, grid, K, "constant coefficients")
    # couplings that are not stored count as 0: two pairs removed, one along axis 0 and one along axis 2
    S = varying_operator(grid, "rand100", 0.3).tolil()
    for i, j in ((100, 101), (200, 272)):
        assert S[i, j] != 0.0
        S[i, j] = 0.0
        S[j, i] = 0.0
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    K = dev.DeviceMultigrid(device_csr_from(S), grid, galerkin=True)
    check_application(S, grid, K, "couplings not stored")
    offs, vals = K.level_operator(0)
    assert vals[1 + offs[1:].index((-1, 0, 0))][101] == 0.0 and vals[1 + offs[1:].index((0, 0, -1))][272] == 0.0


def insert_entry(S, row, col, val):
    """the CSR arrays of S with one more stored entry at the end of `row` (whatever is stored there already)"""
    ind, c, v = S.indptr.copy(), S.indices, S.data
    at = ind[row + 1]
    c = np.concatenate([c[:at], [col], c[at:]]).astype(np.int32)
    v = np.concatenate([v[:at], [val], v[at:]])
    ind[row + 1:] += 1
    return ind.astype(np.int32), c, v


def test_refusals_name_their_reason():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    S = varying_operator(grid, "smooth", 0.3)
    dev.DeviceMultigrid(device_csr_from(S), grid, galerkin=True).close()  # the unchanged matrix is accepted

    def refused(M, why):
        if not isinstance(M, dev.DeviceCSR):
            M = device_csr_from(M) if sp.issparse(M) else dev.DeviceCSR.from_arrays(S.shape, *M)
        with pytest.raises(ValueError, match=why):
            dev.DeviceMultigrid(M, grid, galerkin=True)

    # an entry wrapped across a line end, stored symmetrically: rows 8 and 9 are the end of one line and the start of the next
    P = S.tolil()
    P[8, 9] = -1.0
    P[9, 8] = -1.0
    P = P.tocsr()
    P.sort_indices()
    refused(P, "wraps across a line end")
    # a duplicated entry
    refused(insert_entry(S, 100, 101, S[100, 101]), "stored twice")
    # an unsymmetric pair: one direction differs in the last bit
    P = S.copy()
    k = P.indptr[200] + list(P.indices[P.indptr[200]:P.indptr[201]]).index(201)
    P.data[k] = np.nextafter(P.data[k], 0.0)
    refused(P, "unsymmetric")
    # ... or one direction is not stored at all
    P = S.tolil()
    P[200, 201] = 0.0
    P = P.tocsr()
    P.eliminate_zeros()
    refused(P, "unsymmetric")
    # a missing, a zero and a negative diagonal entry
    at = S.indptr[300] + list(S.indices[S.indptr[300]:S.indptr[301]]).index(300)
    Z = S.copy()
    Z.data[at] = 0.0    # the zero stays stored
    assert Z.nnz == S.nnz
    refused(Z, "diagonal")
    Z = Z.copy()
    Z.eliminate_zeros()
    assert Z[300, 300] == 0.0 and Z.nnz == S.nnz - 1
    refused(Z, "diagonal")
    P = S.copy()
    P.data[at] = -1.0
    refused(P, "diagonal")
    # an offset that is no axis stride (the strides are 1, 9 and 72)
    refused(insert_entry(S, 0, 300, 0.0), "no axis stride")
    # the 2-D operator of (9, 8) passed as (8, 9): the same order, the couplings sit at the wrong strides
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(varying_operator((9, 8), "smooth")), (8, 9), galerkin=True)
    # a handle that gave its index arrays away
    rel = dev.DeviceCSR.poisson(*grid)
    rel.release_arrays()
    refused(rel, "index arrays")
    big = dev.DeviceCSR.poisson_big(*grid)
    refused(big, "index arrays")
    # a matrix on a device list
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0]), (9, 8), galerkin=True)
    # without the new argument the varying matrix is refused as before
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(S), grid)
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(S), grid, galerkin=False)
    # the test hook is for handles that store level operators
    Kc = dev.DeviceMultigrid(dev.DeviceCSR.poisson(*grid), grid)
    with pytest.raises(ValueError):
        Kc.level_operator(0)


# ------------------------------------------------------------------------------------------------ solvers

@functools.lru_cache(maxsize=None)
def oracle_count(grid, kind):
    O = galerkin_oracle_for(grid, kind, 0.0)
    return numpy_pcg(O.A[0], rhs(grid, 11), 1e-8, 200, O.apply)[1]


@pytest.mark.parametrize("kind", ["smooth", "inclusion1e4"])
@pytest.mark.parametrize("grid", [(37, 50), (20, 24, 28)], ids=gid)
def test_pcg_with_the_galerkin_cycle(grid, kind):
    from pysparse_amd import device as dev
    A, S = device_csr(grid, kind, 0.0), galerkin_oracle_for(grid, kind, 0.0).A[0]
    b = rhs(grid, 11)
    K = dev.DeviceMultigrid(A, grid, galerkin=True)
    x = np.zeros(b.size)
    info, it, relres = dev.pcg(A, b, x, 1e-8, 200, K)
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    xj = np.zeros(b.size)
    infoj, itj, _ = dev.pcg(A, b, xj, 1e-8, 5000, dev.DeviceJacobi(A))
    print("pcg %s %s: info %d, %d iterations (oracle-preconditioned NumPy PCG: %d; Jacobi-PCG: %d), true residual %.3e"
          % (grid, kind, info, it, oracle_count(grid, kind), itj, res))
    assert info == 0 and res <= 2e-8
    assert abs(it - oracle_count(grid, kind)) <= 1
    assert infoj == 0 and 4 * it <= itj


@pytest.mark.parametrize("name,grid", [("minres", (37, 50)), ("cgs", (20, 24, 28)), ("bicgstab", (130, 67)),
                                       ("qmrs", (33, 31, 35)), ("gmres", (4100,))])
def test_other_solvers_converge_with_the_handle(name, grid):
    from pysparse_amd import device as dev
    A, S = device_csr(grid, "smooth", 0.0), galerkin_oracle_for(grid, "smooth", 0.0).A[0]
    b = rhs(grid, 13)
    x = np.zeros(b.size)
    info, it, relres = getattr(dev, name)(A, b, x, 1e-8, 100, dev.DeviceMultigrid(A, grid, galerkin=True))
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    print(name, grid, info, it, relres, res)
    assert info == 0 and it <= 40 and res <= 1e-6


@pytest.mark.parametrize("grid", [(37, 50), (20, 24, 28)], ids=gid)
def test_pcg_batch_ends_each_column_as_the_single_solve(grid):
    from pysparse_amd import device as dev
    A = device_csr(grid, "smooth", 0.0)
    n = int(np.prod(grid))
    K = dev.DeviceMultigrid(A, grid, galerkin=True)
    B = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 3)))
    X = np.zeros((n, 3), order="F")
    info, it, relres = dev.pcg_batch(A, B, X, 1e-8, 100, K)
    for c in range(3):
        x = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-8, 100, K)
        assert (info[c], it[c]) == r[:2] and relres[c] == r[2]
        assert np.array_equal(X[:, c], x)


def ll_from(S):
    from pysparse.sparse import spmatrix
    n = S.shape[0]
    L = spmatrix.ll_mat(n, n, S.nnz)
    C_ = S.tocoo()
    for i, j, v in zip(C_.row, C_.col, C_.data):
        L[int(i), int(j)] = float(v)
    return L


def test_jdsym_with_the_galerkin_cycle():
    from pysparse.eigen import jdsym
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    grid = (20, 24)
    S = varying_operator(grid, "smooth", 0.0)
    A = ll_from(S).to_csr()
    K = precon.multigrid(A, grid, galerkin=True)
    assert K.galerkin is True and K.levels == tuple(level_grids(grid))
    kconv, lam, Q, it = jdsym.jdsym(A, None, K, 2, 0.0, 1e-10, 300, krylov.qmrs)[:4]
    spec = np.linalg.eigvalsh(S.toarray())
    assert kconv == 2
    assert np.abs(np.sort(lam) - spec[:2]).max() <= 1e-8


def test_drop_in_solver_takes_it_by_its_handle():
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    grid = (37, 50)
    S = galerkin_oracle_for(grid, "smooth", 0.0).A[0]
    L = ll_from(S)
    b = rhs(grid, 11)
    for A in (L.to_csr(), L):
        x = np.zeros(b.size)
        info, it, relres = krylov.pcg(A, b, x, 1e-8, 100, precon.multigrid(A, grid, galerkin=True))
        assert info == 0 and abs(it - oracle_count(grid, "smooth")) <= 1
        assert np.linalg.norm(b - S @ x) <= 2e-8 * np.linalg.norm(b)
    with pytest.raises(ValueError):  # and without the argument the drop-in module refuses it as before
        precon.multigrid(L.to_csr(), grid)


# ------------------------------------------------------------------------------------------------ structure, threads

@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_level_structure(grid, steps):
    from pysparse_amd import device as dev
    K = dev.DeviceMultigrid(device_csr(grid, "smooth", 0.0), grid, 0.8, steps, galerkin=True)
    lv, tail_first, launches = expected_structure(grid, steps)
    info = K.info()
    assert K.levels == tuple(lv) and info["levels"] == len(lv)
    assert info["tail_first_level"] == tail_first and info["launches_per_apply"] == launches
    assert info["galerkin"] is True


def test_two_threads_with_a_handle_each_on_one_matrix():
    """each thread applies and solves with its own handle, concurrently, on its own stream; both give the bits of the single
    thread"""
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    grid = (33, 31, 35)
    A = device_csr(grid, "rand100", 0.0)
    n = int(np.prod(grid))
    b = rhs(grid, 17)
    Ks = [dev.DeviceMultigrid(A, grid, galerkin=True), dev.DeviceMultigrid(A, grid, galerkin=True)]
    ref_z, ref_x = np.empty(n), np.zeros(n)
    Ks[0].precon(b, ref_z)
    ref_r = dev.pcg(A, b, ref_x, 1e-8, 100, Ks[0])
    assert ref_r[0] == 0
    out, errs, streams = [None, None], [], [None, None]
    start = threading.Barrier(2)

    def worker(k):
        try:
            start.wait()
            got = []
            for _ in range(3):
                z, x = np.empty(n), np.zeros(n)
                Ks[k].precon(b, z)
                r = dev.pcg(A, b, x, 1e-8, 100, Ks[k])
                got.append((z, x, r))
            slot, d, s = C.c_int(-1), C.c_int(-1), C.c_void_p()
            lib().psp_thread_info(C.byref(slot), C.byref(d), C.byref(s))
            streams[k] = s.value
            out[k] = got
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert streams[0] != streams[1]
    for got in out:
        for z, x, r in got:
            assert np.array_equal(z, ref_z) and np.array_equal(x, ref_x) and r == ref_r
