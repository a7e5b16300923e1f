"""GPU: precon.multigrid / device.DeviceMultigrid (psp_mg.hip) against the SciPy oracle of tests/test_multigrid_host.py.

The grids are the smallest that reach each code path: one level only (3, 3, 3); everything inside the single-workgroup
tail; one, two and three levels of launch-per-step kernels above it; odd and even axes; axes that stop coarsening on their
own (64, 64, 3); several tiles of the restriction kernel per level (70, 66, 65); general coefficients and a shift.

The bound on one application is 64 eps max|z|: the float64 oracle lies within 2 eps (relative to max|z|) of the same cycle in
80-bit arithmetic on these grids, 64 eps is 32 times that -- room for any order of the short sums -- and still ten orders of
magnitude below what a wrong weight or a misplaced boundary gives."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from test_multigrid_host import grid_operator, level_grids, numpy_pcg, oracle_for

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TAIL_T = 2048  # the largest level the tail launch takes

GRIDS = [(7,), (64,), (5000,),
         (5, 4), (37, 50), (64, 64), (130, 67),
         (3, 3, 3), (9, 8, 7), (20, 24, 28), (33, 31, 35), (64, 64, 3), (48, 48, 48), (70, 66, 65)]
CASES = [(g, None, 0.0) for g in GRIDS] + [((37, 50), (2.5, 0.7), 0.3), ((20, 24, 28), (4.0, 1.0, 0.5), 0.01)]
IDS = ["x".join(map(str, g)) + ("" if c is None else "-general") for g, c, s in CASES]


def scipy_csr(grid, c, s):
    A = oracle_for(grid, c, s).A[0].copy()
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def device_csr_from(S):
    from pysparse_amd import device as dev
    return dev.DeviceCSR.from_arrays(S.shape, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)


@functools.lru_cache(maxsize=None)
def device_csr(grid, c, s):
    return device_csr_from(scipy_csr(grid, c, s))


def rhs(grid, seed=0):
    return np.random.default_rng(seed).standard_normal(int(np.prod(grid)))


def expected_structure(grid, steps):
    lv = level_grids(grid)
    tail_first = next(l for l, g in enumerate(lv) if int(np.prod(g)) <= TAIL_T)
    # per level above the tail: the pre-smoothing (sweeps one and two are one pass), restriction, prolongation, `steps` sweeps
    launches = 1 + tail_first * ((steps - 1 if steps >= 2 else 1) + 2 + steps)
    return lv, tail_first, launches


# ------------------------------------------------------------------------------------------------ one application

@pytest.mark.parametrize("grid,c,s", CASES, ids=IDS)
def test_one_application_against_the_oracle(grid, c, s):
    from pysparse_amd import device as dev
    A, O = device_csr(grid, c, s), oracle_for(grid, c, s)
    b = rhs(grid)
    worst = 0.0
    for steps in (1, 2, 3):
        for omega in (0.8, 2.0 / 3.0, 1.0):
            K = dev.DeviceMultigrid(A, grid, omega, steps)
            z = np.full(b.size, np.nan)
            K.precon(b, z)
            ref = O.apply(b, omega, steps)
            err = np.abs(z - ref).max() / (EPS * np.abs(ref).max())
            worst = max(worst, err)
            print("grid %s c %s s %s steps %d omega %.4f: max|z - z_oracle| = %.2f eps max|z_oracle|"
                  % (grid, c, s, steps, omega, err))
            assert np.isfinite(z).all() and err <= 64.0, (grid, steps, omega, err)
            K.close()
    print("worst", worst)


@pytest.mark.parametrize("grid", [(1, 1, 600000), (3, 1100000)], ids=["1x1x600000", "3x1100000"])
def test_long_second_and_third_axis(grid):
    """a thin grid whose long axis is not axis 0: the restriction kernel's tiles along axes 1 and 2 are 8 and 4 coarse points
    wide, so these grids need more tiles along that axis than a launch has blocks in y or z -- the tile index rides in x"""
    from pysparse_amd import device as dev
    A, O = device_csr(grid, None, 0.0), oracle_for(grid)
    b = rhs(grid)
    K = dev.DeviceMultigrid(A, grid)
    lv, tail_first, launches = expected_structure(grid, 2)
    info = K.info()
    assert K.levels == tuple(lv) and info["tail_first_level"] == tail_first and info["launches_per_apply"] == launches
    z = np.full(b.size, np.nan)
    K.precon(b, z)
    ref = O.apply(b)
    err = np.abs(z - ref).max() / (EPS * np.abs(ref).max())
    print("grid %s: max|z - z_oracle| = %.2f eps max|z_oracle|" % (grid, err))
    assert np.isfinite(z).all() and err <= 64.0
    x = np.zeros(b.size)
    info_, it, _ = dev.pcg(A, b, x, 1e-8, 200, K)
    S = O.A[0]
    assert info_ == 0 and np.linalg.norm(b - S @ x) <= 2e-8 * np.linalg.norm(b)
    assert abs(it - numpy_pcg(S, b, 1e-8, 200, O.apply)[1]) <= 1


@pytest.mark.parametrize("grid,c,s", CASES, ids=IDS)
def test_same_bits_from_call_to_call_and_from_both_entry_points(grid, c, s):
    from pysparse_amd import device as dev
    A = device_csr(grid, c, s)
    K = dev.DeviceMultigrid(A, grid)
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


@pytest.mark.parametrize("grid,c,s", CASES, ids=IDS)
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_level_structure(grid, c, s, steps):
    from pysparse_amd import device as dev
    K = dev.DeviceMultigrid(device_csr(grid, c, s), grid, 0.8, steps)
    lv, tail_first, launches = expected_structure(grid, steps)
    info = K.info()
    assert K.levels == tuple(lv)
    assert info["levels"] == len(lv)
    assert info["dims"] == tuple(tuple(g) + (1,) * (3 - len(g)) for g in lv)
    assert info["tail_first_level"] == tail_first < info["levels"]  # the tail is engaged
    assert info["launches_per_apply"] == launches


# ------------------------------------------------------------------------------------------------ handle forms

def fill_ll(L, grid, lower_only):
    strides = np.cumprod((1,) + tuple(grid[:-1]))
    n = int(np.prod(grid))
    for k in range(n):
        L[k, k] = 2.0 * len(grid)
        rem = k
        for g, st in zip(grid, strides):
            i = rem % g
            rem //= g
            if i > 0:
                L[k, k - st] = -1.0
            if i < g - 1 and not lower_only:
                L[k, k + st] = -1.0
    return L


def test_handle_forms_give_the_same_bits():
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    from pysparse_amd import device as dev
    grid = (20, 24, 28)
    n = int(np.prod(grid))
    b = rhs(grid, 5)
    ref = np.empty(n)
    dev.DeviceMultigrid(device_csr(grid, None, 0.0), grid).precon(b, ref)
    assert np.abs(ref - oracle_for(grid).apply(b)).max() <= 64 * EPS * np.abs(ref).max()
    ll = fill_ll(spmatrix.ll_mat(n, n, 7 * n), grid, False)
    lls = fill_ll(spmatrix.ll_mat_sym(n, 4 * n), grid, True)
    forms = {"csr_mat": spmatrix.poisson_csr(*grid), "sss_mat": spmatrix.poisson_sss(*grid), "ll_mat": ll,
             "ll_mat.to_csr": ll.to_csr(), "ll_mat_sym.to_sss": lls.to_sss()}
    for name, M in forms.items():
        K = precon.multigrid(M, grid)
        assert K.shape == (n, n) and K.levels == tuple(level_grids(grid)), name
        z = np.empty(n)
        K.precon(b, z)
        assert np.array_equal(z, ref), name
    big = dev.DeviceCSR.poisson_big(*grid)
    z = np.empty(n)
    dev.DeviceMultigrid(big, grid).precon(b, z)
    assert np.array_equal(z, ref)
    rel = dev.DeviceCSR.poisson(*grid)
    rel.release_arrays()
    z = np.empty(n)
    dev.DeviceMultigrid(rel, grid).precon(b, z)
    assert np.array_equal(z, ref)
    sss = dev.DeviceSSS.poisson(*grid)
    z = np.empty(n)
    dev.DeviceMultigrid(sss, grid).precon(b, z)
    assert np.array_equal(z, ref)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals():
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    S = scipy_csr(grid, None, 0.0)
    dev.DeviceMultigrid(device_csr_from(S), grid).close()  # the unchanged matrix is accepted
    # one perturbed value (an interior row, so that row 0 still names the stencil)
    P = S.copy()
    P.data[P.indptr[200] + 1] *= 1.0 + 2.0 ** -40
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(P), grid)
    # a variable coefficient on the diagonal of the last row
    P = S.copy()
    P.data[P.indptr[-1] - 1] += 0.5
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(P), grid)
    # one extra stored entry: the coupling across a line end between rows 8 and 9 of the first plane, one direction only
    P = S.tolil()
    P[8, 9] = -1.0
    P = P.tocsr()
    P.sort_indices()
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(P), grid)
    # an explicitly stored zero where the stencil has nothing
    ind, col, val = S.indptr.copy(), S.indices.copy(), S.data.copy()
    col = np.concatenate([col[:ind[1]], [300], col[ind[1]:]]).astype(np.int32)
    val = np.concatenate([val[:ind[1]], [0.0], val[ind[1]:]])
    ind[1:] += 1
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(dev.DeviceCSR.from_arrays(S.shape, ind.astype(np.int32), col, val), grid)
    # a missing entry
    P = S.tolil()
    P[100, 101] = 0.0
    P = P.tocsr()
    P.eliminate_zeros()
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(P), grid)
    # 1-D Poisson of n0 n1 rows passed as a 2-D grid: couplings across line ends, none along the second axis
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr(( 72,), None, 0.0), (9, 8))
    # ... and the 2-D operator of (9, 8) passed as (8, 9)
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr((9, 8), None, 0.0), (8, 9))
    # a negative shift
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(scipy_csr(grid, None, -0.1)), grid)
    # positive couplings
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(device_csr_from(scipy_csr((9, 8), (-1.0, 1.0), 8.0)), (9, 8))
    # a matrix on a device list
    M = dev.DeviceCSR.poisson_multi(9, 8, devices=[0, 0])
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(M, (9, 8))
    # the same through the index-free layout: a shifted diagonal is a constant stencil (accepted), a banded matrix with
    # couplings across line ends is not
    big = dev.DeviceCSR.poisson_big(9, 8, 7)
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(big, (8, 9, 7))
    with pytest.raises(ValueError):
        dev.DeviceMultigrid(big, (72, 7))


def test_drop_in_module_raises_value_error_for_a_wrong_matrix():
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    A = spmatrix.poisson_csr(9, 8)
    with pytest.raises(ValueError):
        precon.multigrid(A, (8, 9))
    L = fill_ll(spmatrix.ll_mat(72, 72, 5 * 72), (9, 8), False)
    L[5, 5] = 4.5
    with pytest.raises(ValueError):
        precon.multigrid(L, (9, 8))


# ------------------------------------------------------------------------------------------------ solves

@functools.lru_cache(maxsize=None)
def oracle_counts(grid, c, s):
    O = oracle_for(grid, c, s)
    A = O.A[0]
    b = rhs(grid, 11)
    _, it = numpy_pcg(A, b, 1e-8, 200, O.apply)
    return it


@pytest.mark.parametrize("grid,c,s", CASES, ids=IDS)
def test_pcg_and_minres_with_multigrid(grid, c, s):
    from pysparse_amd import device as dev
    A, S = device_csr(grid, c, s), oracle_for(grid, c, s).A[0]
    n = S.shape[0]
    b = rhs(grid, 11)
    K = dev.DeviceMultigrid(A, grid)
    tol = 1e-8
    x = np.zeros(n)
    info, it, relres = dev.pcg(A, b, x, tol, 200, K)
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    it_oracle = oracle_counts(grid, c, s)
    print("pcg %s: info %d, %d iterations (oracle-preconditioned NumPy PCG: %d), true residual %.3e"
          % (grid, info, it, it_oracle, res))
    assert info == 0 and res <= 2 * tol
    assert abs(it - it_oracle) <= 1
    if n > 1000:
        xj = np.zeros(n)
        infoj, itj, _ = dev.pcg(A, b, xj, tol, 2 * n, dev.DeviceJacobi(A))
        print("    Jacobi-PCG: %d iterations" % itj)
        assert infoj == 0 and 4 * it <= itj
    xm = np.zeros(n)
    infom, itm, _ = dev.minres(A, b, xm, tol, 200, K)
    resm = np.linalg.norm(b - S @ xm) / np.linalg.norm(b)
    print("minres %s: info %d, %d iterations, true residual %.3e" % (grid, infom, itm, resm))
    assert infom == 0 and resm <= 2 * tol


@pytest.mark.parametrize("grid", [(37, 50), (20, 24, 28)], ids=["37x50", "20x24x28"])
def test_pcg_batch_ends_each_column_as_the_single_solve(grid):
    from pysparse_amd import device as dev
    A = device_csr(grid, None, 0.0)
    n = int(np.prod(grid))
    K = dev.DeviceMultigrid(A, grid)
    B = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 3)))
    X = np.zeros((n, 3), order="F")
    info, it, relres = dev.pcg_batch(A, B, X, 1e-8, 100, K)
    for c in range(3):
        x = np.zeros(n)
        r = dev.pcg(A, np.ascontiguousarray(B[:, c]), x, 1e-8, 100, K)
        assert (info[c], it[c]) == r[:2] and relres[c] == r[2]
        assert np.array_equal(X[:, c], x)


@pytest.mark.parametrize("name", ["cgs", "bicgstab", "qmrs", "gmres"])
def test_other_solvers_converge_with_multigrid(name):
    from pysparse_amd import device as dev
    grid = (33, 31, 35)
    A, S = device_csr(grid, None, 0.0), oracle_for(grid).A[0]
    b = rhs(grid, 13)
    x = np.zeros(b.size)
    info, it, relres = getattr(dev, name)(A, b, x, 1e-8, 100, dev.DeviceMultigrid(A, grid))
    res = np.linalg.norm(b - S @ x) / np.linalg.norm(b)
    print(name, info, it, relres, res)
    assert info == 0 and it <= 30 and res <= 1e-6


def test_jdsym_with_multigrid():
    from pysparse.eigen import jdsym
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    nx, ny = 20, 24
    A = spmatrix.poisson_csr(nx, ny)
    K = precon.multigrid(A, (nx, ny))
    kconv, lam, Q, it = jdsym.jdsym(A, None, K, 3, 0.0, 1e-10, 300, krylov.qmrs)[:4]
    p, q = np.arange(1, nx + 1), np.arange(1, ny + 1)
    spec = np.sort((4 - 2 * np.cos(p * np.pi / (nx + 1)))[:, None] - 2 * np.cos(q * np.pi / (ny + 1))[None, :], axis=None)
    assert kconv == 3
    assert np.abs(np.sort(lam) - spec[:3]).max() <= 1e-8


def test_drop_in_solver_takes_it_by_its_handle():
    from pysparse.itsolvers import krylov
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    grid = (37, 50)
    A = spmatrix.poisson_csr(*grid)
    K = precon.multigrid(A, grid)
    b = rhs(grid, 11)
    x = np.zeros(b.size)
    info, it, relres = krylov.pcg(A, b, x, 1e-8, 100, K)
    assert info == 0 and abs(it - oracle_counts(grid, None, 0.0)) <= 1
    S = oracle_for(grid).A[0]
    assert np.linalg.norm(b - S @ x) <= 2e-8 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------------------ threads

def test_two_threads_with_a_handle_each_on_one_matrix():
    """each thread applies and solves with its own handle, concurrently, on its own stream; both give the bits of the single
    thread.  (Their overlap in time is asserted by test_two_threads_two_multigrid_handles_overlap below, in a fresh
    interpreter.)"""
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    grid = (70, 66, 65)
    A = device_csr(grid, None, 0.0)
    n = int(np.prod(grid))
    b = rhs(grid, 17)
    Ks = [dev.DeviceMultigrid(A, grid), dev.DeviceMultigrid(A, grid)]
    ref_z, ref_x = np.empty(n), np.zeros(n)
    Ks[0].precon(b, ref_z)
    ref_r = dev.pcg(A, b, ref_x, 1e-8, 100, Ks[0])
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


def test_two_threads_two_multigrid_handles_overlap():
    """two handles on ONE matrix, a thread each: side by side they take clearly less wall-clock time than one after the
    other, and give the same bits.  (In a fresh interpreter, like tests/test_gpu_threads.py: whether two streams overlap on
    the device also depends on which hardware queues the runtime maps them to, in the order the process created its
    streams; after hundreds of other tests in the same process the two threads' streams can share one.)"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, PSP_TEST_MG_OVERLAP_CHILD="1")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", here, "-k", "mg_overlap_child"], env=env,
                       cwd=os.path.dirname(os.path.dirname(here)), capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.skipif(__import__("os").environ.get("PSP_TEST_MG_OVERLAP_CHILD") != "1", reason="runs in the child of the test above")
def test_mg_overlap_child():
    import time
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    L = lib()
    # a size at which a cycle is a chain of short dependent launches (two launch-per-step levels and the tail): the GPU is
    # far from full, so two streams side by side must beat one after the other
    grid = (48, 48, 48)
    A = device_csr(grid, None, 0.0)
    n = int(np.prod(grid))
    b = rhs(grid, 19)
    Ks = [dev.DeviceMultigrid(A, grid), dev.DeviceMultigrid(A, grid)]
    bufs = [(dev.DeviceBuffer.from_host(b), dev.DeviceBuffer(n)) for _ in range(2)]
    reps = 3000

    def work(k):
        xb, yb = bufs[k]
        for _ in range(reps):
            Ks[k].precon_dev(xb.ptr, yb.ptr)
        L.psp_synchronize()

    ref = np.empty(n)
    Ks[0].precon(b, ref)
    for k in range(2):  # warm-up
        work(k)
    t = time.perf_counter()
    for k in range(2):
        work(k)
    t_serial = time.perf_counter() - t
    errs, streams = [], [None, None]
    start = threading.Barrier(2)

    def worker(k):
        try:
            slot, d, s = C.c_int(-1), C.c_int(-1), C.c_void_p()
            L.psp_thread_info(C.byref(slot), C.byref(d), C.byref(s))
            streams[k] = s.value
            start.wait()
            work(k)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    t = time.perf_counter()
    [x.start() for x in ts]
    [x.join() for x in ts]
    t_threads = time.perf_counter() - t
    assert not errs, errs
    assert streams[0] and streams[1] and streams[0] != streams[1]  # two streams of their own, not the null stream
    for xb, yb in bufs:
        assert np.array_equal(yb.download(), ref)  # the bits of a single call through the host-vector entry point
    print("two multigrid handles, %d applications each: one after the other %.1f ms, side by side %.1f ms (%.2f)"
          % (reps, 1e3 * t_serial, 1e3 * t_threads, t_threads / t_serial))
    # overlap: side by side clearly faster than one after the other (ideally the longer of the two = half)
    assert t_threads < 0.85 * t_serial, (t_threads, t_serial)
