"""GPU: the block V-cycle of precon.multigrid (psp_mg_precon_block / _dev, psp_mg_block_reserve / _info; DESIGN.md
section 9e) and psp_pcg_batch with a multigrid K.

The contract is section 9b's, column by column: column c of a block application has the bits of psp_mg_precon on column
c, in both modes (matrix-free and galerkin=True), for every `steps`, handle form and entry point.  No tolerance anywhere.

The grids are those of tests/test_gpu_multigrid_galerkin.py, the smallest that reach each way to go wrong: two
launch-per-step levels in 1-D (4100,); everything inside the tail, where the block form is gridDim.x = k only
(9, 8, 7); a 9-point level just above the tail (130, 67); semi-coarsening (16, 16, 3); a grid that crosses the
restriction tile in every axis with a 27-point level above the tail (33, 31, 35)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import grid_operator, level_grids
from test_multigrid_galerkin_host import varying_operator

pytestmark = pytest.mark.gpu

GRIDS = [(4100,), (9, 8, 7), (130, 67), (16, 16, 3), (33, 31, 35)]
MODES = ["poisson", "smooth", "rand1e4"]  # the matrix-free mode on the Poisson operator, galerkin=True on the other two
KS = (1, 2, 3, 4, 5, 9)
KMAX = max(KS)
PAD = 5
# columns per thread of the sweep, scale and prolongation kernels (psp_mg.hip kBlockKCMatrixFree / kBlockKCGalerkin)
KC = {"poisson": 2, "smooth": 4, "rand1e4": 4}
LOOP_OWN = 7  # psp_batch.hip beside the cycle: r.z, head, pupdate, product, finish, xr, finish
EINVAL = -1


def gid(g):
    return "x".join(map(str, g))


@functools.lru_cache(maxsize=None)
def operator(grid, mode):
    if mode == "poisson":
        A = grid_operator(grid, (1.0,) * len(grid), 0.0).copy()
        A.sum_duplicates()
        A.eliminate_zeros()
    else:
        A = varying_operator(grid, mode, 0.0)
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def device_csr(grid, mode):
    from pysparse_amd import device as dev
    S = operator(grid, mode)
    return dev.DeviceCSR.from_arrays(S.shape, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)


@functools.lru_cache(maxsize=None)
def device_sss(grid, mode):
    from pysparse_amd import device as dev
    S = operator(grid, mode)
    L = sp.tril(S, -1, format="csr")
    L.sort_indices()
    return dev.DeviceSSS.from_arrays(S.shape[0], L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data,
                                     S.diagonal().copy())


def multigrid(A, grid, mode, steps=2):
    from pysparse_amd import device as dev
    return dev.DeviceMultigrid(A, grid, 0.8, steps, galerkin=mode != "poisson")


def columns(n, k, seed=0):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, k)))


def singles(K, X):
    """precon on every column: the reference, computed once per handle"""
    n, k = X.shape
    Z = np.empty((n, k), order="F")
    z = np.empty(n)
    for c in range(k):
        K.precon(np.ascontiguousarray(X[:, c]), z)
        Z[:, c] = z
    return Z


def padded(X, k):
    """(the whole array, its view of the first n rows): leading dimension n + PAD, the padding filled with NaN"""
    n = X.shape[0]
    big = np.full((n + PAD, k), np.nan, order="F")
    big[:n] = X[:, :k]
    return big, big[:n]


def block_dev(K, X, k):
    """the device entry point on blocks of leading dimension n + PAD; returns Y's whole array and X's after the call"""
    from pysparse_amd import device as dev
    n = X.shape[0]
    xbig, _ = padded(X, k)
    xd = dev.DeviceBuffer.from_host(xbig.ravel(order="F"))
    yd = dev.DeviceBuffer.from_host(np.full((n + PAD) * k, np.nan))
    K.precon_block_dev(k, xd.ptr, n + PAD, yd.ptr, n + PAD)
    y = yd.download().reshape((n + PAD, k), order="F")
    x = xd.download().reshape((n + PAD, k), order="F")
    xd.free()
    yd.free()
    return y, x


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def check_block(K, X, Z, k, tag):
    """host entry point on padded views: the singles' bits, padding untouched, X unchanged, twice the same"""
    n = X.shape[0]
    xbig, xv = padded(X, k)
    ybig, yv = padded(np.zeros((n, k)), k)
    yv[...] = np.nan
    K.precon_block(xv, yv)
    for c in range(k):
        assert np.array_equal(yv[:, c], Z[:, c]), (tag, k, c)
    assert np.isnan(ybig[n:]).all() and np.isnan(xbig[n:]).all(), (tag, k)
    assert np.array_equal(xv, X[:, :k]), (tag, k)
    again = np.full((n, k), np.nan, order="F")
    K.precon_block(xv, again)
    assert same_bits(again, np.asfortranarray(yv)), (tag, k)
    return yv


# ------------------------------------------------------------------------------------------------ 1: block == singles

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", GRIDS, ids=gid)
def test_block_application_equals_single_applications(grid, mode):
    n = int(np.prod(grid))
    X = columns(n, KMAX, 3)
    for steps in (1, 2, 3):
        K = multigrid(device_csr(grid, mode), grid, mode, steps)
        Ks = multigrid(device_sss(grid, mode), grid, mode, steps)
        Z = singles(K, X)
        assert np.isfinite(Z).all() and np.abs(Z).max() > 0.0
        launches = K.info()["launches_per_apply"]
        for k in KS:
            yv = check_block(K, X, Z, k, (grid, mode, steps, "csr"))
            ys = np.full((n, k), np.nan, order="F")
            Ks.precon_block(np.asfortranarray(X[:, :k]), ys)
            assert same_bits(ys, np.asfortranarray(yv)), (grid, mode, steps, k, "sss")
            yd, xd = block_dev(K, X, k)
            assert same_bits(np.asfortranarray(yd[:n]), np.asfortranarray(yv)), (grid, mode, steps, k, "device")
            assert np.isnan(yd[n:]).all() and np.array_equal(xd[:n], X[:, :k]) and np.isnan(xd[n:]).all()
            assert K.info()["launches_per_apply"] == launches
        K.close()
        Ks.close()


def test_any_strides_and_the_drop_in_object():
    """C-ordered and strided (n, k) arrays are staged like matmat's; precon.multigrid's object has the same method"""
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    grid, mode = (130, 67), "smooth"
    n = int(np.prod(grid))
    X = columns(n, 5, 4)
    K = multigrid(device_csr(grid, mode), grid, mode)
    Z = singles(K, X)
    Xc = np.ascontiguousarray(X)          # row-major
    Yc = np.full((n, 5), np.nan)
    K.precon_block(Xc, Yc)
    assert np.array_equal(Yc, Z)
    wide = np.full((n, 10), np.nan, order="F")
    K.precon_block(X, wide[:, ::2])       # every other column of a wider block
    assert np.array_equal(wide[:, ::2], Z) and np.isnan(wide[:, 1::2]).all()
    with pytest.raises(ValueError):
        K.precon_block(X, np.empty((n, 4)))
    S = operator(grid, mode).tocoo()
    L = spmatrix.ll_mat(n, n, S.nnz)
    for i, j, v in zip(S.row, S.col, S.data):
        L[int(i), int(j)] = float(v)
    Kd = precon.multigrid(L.to_csr(), grid, galerkin=True)
    Yd = np.full((n, 5), np.nan)
    Kd.precon_block(Xc, Yd)
    assert np.array_equal(Yd, Z)
    with pytest.raises(ValueError):
        Kd.precon_block(Xc, np.empty((n, 4)))


# ------------------------------------------------------------------------------------------------ 2: group boundaries

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", [(33, 31, 35), (4100,)], ids=gid)
def test_column_group_boundaries(grid, mode):
    """k = KC (one full group), KC + 1 (a remainder group of one) and 2 KC + 1 (two full groups in gridDim.y and the
    remainder), with the mode's KC; the restriction and the tail take a column per workgroup"""
    n = int(np.prod(grid))
    kc = KC[mode]
    X = columns(n, 2 * kc + 1, 5)
    K = multigrid(device_csr(grid, mode), grid, mode)
    Z = singles(K, X)
    for k in (kc, kc + 1, 2 * kc + 1):
        check_block(K, X, Z, k, (grid, mode))
        yd, _ = block_dev(K, X, k)
        assert np.array_equal(yd[:n], Z[:, :k])
    K.close()


# ------------------------------------------------------------------------------------------------ 3: frozen columns

def smooth_column(grid):
    v = np.ones(1)
    for m in grid:  # axis 0 is the fastest index
        v = np.outer(np.sin(np.pi * np.arange(1, m + 1) / (m + 1)), v).ravel()
    return v


class System:
    """B and X0 with the column set of tests/test_gpu_pcg_batch.py, and the single solves, each computed once"""

    def __init__(self, grid, mode):
        self.grid, self.mode = grid, mode
        self.A = device_csr(grid, mode)
        self.K = multigrid(self.A, grid, mode)
        S = operator(grid, mode)
        n = self.n = S.shape[0]
        rng = np.random.default_rng(7)
        B = rng.standard_normal((n, KMAX))
        X0 = np.zeros((n, KMAX))
        B[:, 0] = S @ np.ones(n)
        B[:, 2] = 0.0
        X0[:, 2] = rng.standard_normal(n)  # must come back as zeros
        X0[:, 3] = rng.standard_normal(n)  # already the solution
        y = np.empty(n)
        self.A.matvec(np.ascontiguousarray(X0[:, 3]), y)
        B[:, 3] = y
        B[:, 4] = S @ smooth_column(grid)  # converges early beside the rough ones
        X0[:, 6] = rng.standard_normal(n)  # a nonzero initial guess
        self.B, self.X0 = B, X0
        self.single = {}

    def alone(self, c, maxit):
        from pysparse_amd.device import pcg
        if (c, maxit) not in self.single:
            x = np.ascontiguousarray(self.X0[:, c])
            res = pcg(self.A, np.ascontiguousarray(self.B[:, c]), x, 1e-8, maxit, self.K)
            self.single[(c, maxit)] = (res, x)
        return self.single[(c, maxit)]


@functools.lru_cache(maxsize=None)
def system(grid, mode):
    return System(grid, mode)


def check_batch(S, k, maxit):
    from pysparse_amd.device import pcg_batch
    n = S.n
    xbig, X = padded(S.X0, k)
    bbig, B = padded(S.B, k)
    info, it, rr = pcg_batch(S.A, B, X, 1e-8, maxit, S.K)
    assert np.isnan(xbig[n:]).all() and np.array_equal(B, S.B[:, :k])
    for c in range(k):
        (i1, it1, rr1), x1 = S.alone(c, maxit)
        print(S.grid, S.mode, "k", k, "maxit", maxit, "col", c, "batch", (info[c], it[c], rr[c]), "alone", (i1, it1, rr1))
        assert info[c] == i1 and it[c] == it1, (c, k)
        assert float(rr[c]) == float(rr1), (c, k)
        assert np.array_equal(X[:, c], x1), (c, k)
    return info, it


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", [(37, 50), (20, 24, 28)], ids=gid)
def test_pcg_batch_with_frozen_columns(grid, mode):
    S = system(grid, mode)
    for k in (5, 9):
        info, it = check_batch(S, k, 100)
        assert (info == 0).all()
        assert it[2] == 0 and it[3] == 0 and it[0] > 0 and it[1] > 0  # frozen from the start beside running ones
    for k in (5, 9):
        info, it = check_batch(S, k, 3)
        assert info[1] == -1 and it[1] == 4  # ran out
        assert info[2] == 0 and info[3] == 0


# ------------------------------------------------------------------------------------------------ 4: launches

@pytest.mark.parametrize("mode", ["poisson", "smooth"])
def test_launches_do_not_grow_with_k(mode):
    from pysparse_amd.device import last_solve_info, pcg_batch
    S = system((20, 24, 28), mode)
    per_apply = S.K.info()["launches_per_apply"]
    seen = []
    for k in (2, 9):
        X = np.asfortranarray(S.X0[:, :k].copy())
        B = np.asfortranarray(S.B[:, :k].copy())
        pcg_batch(S.A, B, X, 1e-8, 100, S.K)
        name, d = last_solve_info()
        assert name == "pcg_batch"
        seen.append(d["launches"])
    assert seen[0] == seen[1] and seen[0] > 0
    assert seen[0] == per_apply + LOOP_OWN


# ------------------------------------------------------------------------------------------------ 5: storage, refusals

def test_block_storage():
    from pysparse_amd._capi import lib
    grid, mode = (33, 31, 35), "smooth"
    n = int(np.prod(grid))
    X = columns(n, 5, 6)
    K = multigrid(device_csr(grid, mode), grid, mode)
    Z = singles(K, X)
    assert K.block_info() == {"columns": 0, "bytes": 0}
    Y = np.empty((n, 2), order="F")
    K.precon_block(np.asfortranarray(X[:, :2]), Y)
    two = K.block_info()
    # what the single cycle keeps, per column: a spare for every level above the tail, x and b for every level but the finest
    # down to the one that heads the tail
    lv = [int(np.prod(g)) for g in level_grids(grid)]
    tf = K.info()["tail_first_level"]
    per_column = 8 * (sum(lv[:tf]) + 2 * sum(lv[1:tf + 1]))
    assert two == {"columns": 2, "bytes": 2 * per_column}
    Y5 = np.empty((n, 5), order="F")
    K.precon_block(X, Y5)
    assert K.block_info() == {"columns": 5, "bytes": 5 * per_column}
    K.precon_block(np.asfortranarray(X[:, :2]), Y)  # fewer columns: nothing shrinks
    assert K.block_info()["columns"] == 5
    assert lib().psp_mg_block_reserve(K._h, 0) == 0
    assert K.block_info() == {"columns": 0, "bytes": 0}
    K.block_reserve(7)
    assert K.block_info() == {"columns": 7, "bytes": 7 * per_column}
    K.block_reserve(0)
    Y5b = np.empty((n, 5), order="F")
    K.precon_block(X, Y5b)
    assert same_bits(Y5, Y5b) and np.array_equal(Y5, Z) and np.array_equal(Y[:, :2], Z[:, :2])
    assert lib().psp_mg_block_reserve(K._h, -1) == EINVAL
    K.close()


def test_refusals():
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    grid, mode = (130, 67), "poisson"
    n = int(np.prod(grid))
    K = multigrid(device_csr(grid, mode), grid, mode)
    k = 3
    xd = dev.DeviceBuffer.from_host(np.zeros((n + PAD) * k))
    yd = dev.DeviceBuffer.from_host(np.zeros((n + PAD) * k))
    L = lib()
    ld = n + PAD
    assert L.psp_mg_precon_block_dev(K._h, k, xd.ptr, ld, yd.ptr, ld) == 0
    assert L.psp_mg_precon_block_dev(K._h, k, xd.ptr, ld, xd.ptr, ld) == EINVAL            # aliased
    assert L.psp_mg_precon_block_dev(K._h, 1, xd.ptr, ld, xd.ptr + 8 * (n - 1), ld) == EINVAL  # overlapping by one element
    assert L.psp_mg_precon_block_dev(K._h, 0, xd.ptr, ld, yd.ptr, ld) == EINVAL            # k < 1
    assert L.psp_mg_precon_block_dev(K._h, -2, xd.ptr, ld, yd.ptr, ld) == EINVAL
    assert L.psp_mg_precon_block_dev(K._h, k, xd.ptr, n - 1, yd.ptr, ld) == EINVAL         # short leading dimensions
    assert L.psp_mg_precon_block_dev(K._h, k, xd.ptr, ld, yd.ptr, n - 1) == EINVAL
    assert L.psp_mg_precon_block_dev(K._h, k, None, ld, yd.ptr, ld) == EINVAL
    xh, yh = np.zeros((n, k), order="F"), np.zeros((n, k), order="F")
    assert L.psp_mg_precon_block(K._h, k, xh.ctypes.data_as(C.c_void_p), n, xh.ctypes.data_as(C.c_void_p), n) == EINVAL
    assert L.psp_mg_precon_block(K._h, 0, xh.ctypes.data_as(C.c_void_p), n, yh.ctypes.data_as(C.c_void_p), n) == EINVAL
    assert L.psp_mg_precon_block(K._h, k, xh.ctypes.data_as(C.c_void_p), n - 1, yh.ctypes.data_as(C.c_void_p), n) == EINVAL
    with pytest.raises(ValueError):
        K.precon_block_dev(k, xd.ptr, ld, xd.ptr, ld)
    xd.free()
    yd.free()
    K.close()


# ------------------------------------------------------------------------------------------------ 6: the retired switch

RETIRED_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
from pysparse_amd import device as dev
from test_gpu_multigrid_block import columns, device_csr, singles
grid, k = (36, 34, 33), 5
n = int(np.prod(grid))
X = columns(n, k, 9)
for mode in ("poisson", "smooth"):
    for cls in (dev.DeviceMultigrid, dev.DeviceMultigrid32):
        K = cls(device_csr(grid, mode), grid, 0.8, 2, galerkin=mode != "poisson")
        info = K.info()
        assert [int(np.prod(d)) for d in info["dims"][:3]] == [40392, 4896, 576] and info["tail_first_level"] == 2, info
        Z = singles(K, X)
        assert np.isfinite(Z).all() and np.abs(Z).max() > 0.0
        Y = np.full((n, k), np.nan, order="F")
        K.precon_block(X, Y)
        for c in range(k):
            assert np.array_equal(Y[:, c].view(np.int64), Z[:, c].view(np.int64)), (mode, info["precision"], c)
        print("same bits", mode, info["precision"])
        K.close()
"""


def test_retired_restriction_switch_is_inert():
    """PSP_MG_BLOCK_KCR (2 or 4 residual tiles per workgroup of the block restriction) is gone: a fresh process started
    with PSP_TUNING=1 PSP_MG_BLOCK_KCR=4 still gives every column of precon_block the bits of precon on that column.  The
    grid (36, 34, 33) is the smallest with two launch-per-step levels (40392 and 4896 points above the 576-point tail), so
    the restriction runs on a level-0 shape and on a full 13-offset shape; k = 5 leaves a KC = 4 group a remainder
    column; both modes, both precisions."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSP_TUNING="1", PSP_MG_BLOCK_KCR="4")
    p = subprocess.run([sys.executable, "-c", RETIRED_CHILD % (root, os.path.join(root, "tests"))], env=env,
                       capture_output=True, text=True, cwd=root, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    for mode in ("poisson", "smooth"):
        for precision in ("double", "single"):
            assert "same bits %s %s" % (mode, precision) in p.stdout, p.stdout


def test_two_threads_with_a_handle_each_on_one_matrix():
    grid, mode = (33, 31, 35), "rand1e4"
    n = int(np.prod(grid))
    A = device_csr(grid, mode)
    X = columns(n, 5, 8)
    Ks = [multigrid(A, grid, mode), multigrid(A, grid, mode)]
    Z = singles(Ks[0], X)
    out, errs = [None, None], []
    start = threading.Barrier(2)

    def worker(t):
        try:
            start.wait()
            got = []
            for k in (5, 3, 5):
                Y = np.full((n, k), np.nan, order="F")
                Ks[t].precon_block(np.asfortranarray(X[:, :k]), Y)
                got.append(Y)
            out[t] = got
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for got in out:
        for Y in got:
            assert np.array_equal(Y, Z[:, :Y.shape[1]])
