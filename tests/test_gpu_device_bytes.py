"""GPU: a precon.ssor or precon.multigrid handle gives back the device memory it took (psp_debug_device_bytes; DESIGN.md
section 8).  Every case reads the bytes the library's owning arrays hold, creates a handle (the count grows), uses it
once, closes it and finds the first value again -- before and after psp_trim, which has no part in it.  A creation that is
refused half-way, after levels, vectors or a brick plan were allocated, raises what it raises in the tests it is taken
from and leaves the count where it was.

The SSOR operators are one per schedule the set-up can produce: the slot-major (ELL) form with runs of narrow levels
(poisson2d(100)), pipelined bricks (the 100 x 90 x 80 grid of test_ssor_bricks_bit_exact), a grid operator with a coupling
across a line end, which is examined for bricks and refused before a plan is made (the matrix of
test_ssor_bricks_refuse_what_is_not_a_grid_operator), a grid operator with couplings missing, for which a brick plan is made,
found infeasible and dropped (the 96^3 operator of test_ssor_bricks_bit_exact with keep = 0.97), and per-level launches on rows of up to 12 entries (the `random`
operator of test_ssor_precon_bit_exact).  The multigrid grids (33, 17, 9) and (70, 45) have levels above the tail launch."""
import functools
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_box_host import box_operator
from test_multigrid_galerkin_host import varying_operator
from test_multigrid_interp_host import interp_operator
from test_multigrid_line_host import graded_operator
import test_gpu_multigrid_galerkin as gk
import test_gpu_ssor as ss

pytestmark = pytest.mark.gpu


def counters():
    from pysparse_amd import device as dev
    return dev.debug_device_bytes()


def live_bytes():
    return counters()[0]


def start():
    """the counters before a case; handles that earlier tests left to the collector are closed first, so that none of
    them goes while the case is counting"""
    gc.collect()
    return counters()


def returned(base):
    """the count is `base` again, whether or not the pools are trimmed"""
    from pysparse_amd._capi import lib
    assert live_bytes() == base
    assert lib().psp_trim() == 0
    assert live_bytes() == base


# ------------------------------------------------------------------------------------------------ precon.ssor

@functools.lru_cache(maxsize=None)
def ssor_operator(which):
    from oracle import oracle as O
    from pysparse_amd.device import DeviceSSS
    if which == "runs":
        S = O.poisson_sss(100, 100)
    elif which == "bricks":
        S = ss.grid_sss(O, 100, 90, 80, seed=11 + 270, keep=1.0)
    elif which == "not-a-grid":
        G = ss.grid_sss(O, 128, 128, 64, seed=5, keep=1.0)
        r = 128  # first point of the second grid line: its offset -1 neighbour is the end of the first line
        hi = G.ind[r + 1]
        ind = G.ind.copy()
        ind[r + 1:] += 1
        S = O.SSS(G.n, np.insert(G.val, hi, -0.25), G.diag, np.insert(G.col, hi, r - 1), ind)
    elif which == "plan-dropped":
        S = ss.grid_sss(O, 96, 96, 96, seed=11 + 288, keep=0.97)
    else:
        S = ss.random_sss(O, 2500, 11)
    return S.n, DeviceSSS.from_arrays(S.n, S.ind, S.col, S.val, S.diag)


@pytest.mark.parametrize("omega", [1.0, 1.3])
@pytest.mark.parametrize("which", ["runs", "bricks", "not-a-grid", "plan-dropped", "levels"])
def test_an_ssor_handle_returns_what_it_took(which, omega):
    from pysparse_amd.device import DeviceSSOR
    n, D = ssor_operator(which)
    base, made = start()
    K = DeviceSSOR(D, omega, 1)
    held, made_now = counters()
    assert held > base and made_now > made
    assert (K.bricks > 0) == (which == "bricks")
    if which == "runs":
        assert K.lds_runs[0] > 0 and K.lds_runs[1] > 0
    if which == "levels":
        assert K.lds_runs == (0, 0, 0, 0)
    x, y = ss.rng_vec(n, 3), np.zeros(n)
    K.precon(x, y)
    assert np.isfinite(y).all() and y.any()
    assert live_bytes() == held  # the host-pointer call's staging is gone again
    K.close()
    returned(base)


# ------------------------------------------------------------------------------------------------ precon.multigrid

MG_GRIDS = [(33, 17, 9), (70, 45)]
MG_MODES = ["matrix-free", "matrix-free-single", "galerkin", "galerkin-single", "line", "box", "interp"]


@functools.lru_cache(maxsize=None)
def mg_operator(grid, box):
    from pysparse_amd import device as dev
    if box:
        return gk.device_csr_from(box_operator(grid, "q1kappa"))
    return dev.DeviceCSR.poisson(*grid)


def mg_handle(mode, A, grid):
    from pysparse_amd import device as dev
    if mode == "matrix-free":
        return dev.DeviceMultigrid(A, grid)
    if mode == "matrix-free-single":
        return dev.DeviceMultigrid32(A, grid)
    if mode == "galerkin":
        return dev.DeviceMultigrid(A, grid, galerkin=True)
    if mode == "galerkin-single":
        return dev.DeviceMultigrid32(A, grid, galerkin=True)
    if mode == "line":
        return dev.DeviceMultigridLine(A, grid, line=1)
    if mode == "box":
        return dev.DeviceMultigridBox(A, grid)
    return dev.DeviceMultigridInterp(A, grid)


@pytest.mark.parametrize("mode", MG_MODES)
@pytest.mark.parametrize("grid", MG_GRIDS, ids=gk.gid)
def test_a_multigrid_handle_returns_what_it_took(grid, mode):
    A = mg_operator(grid, mode == "box")
    n = int(np.prod(grid))
    base = start()[0]
    K = mg_handle(mode, A, grid)
    held = live_bytes()
    at_rest = K.bytes()
    assert held - base == at_rest["operator"] + at_rest["vector"]  # what psp_mg_bytes reports is what the handle holds
    b, z = gk.rhs(grid, 5), np.empty(n)
    K.precon(b, z)
    assert np.isfinite(z).all() and z.any()
    B = np.asfortranarray(np.random.default_rng(6).standard_normal((n, 3)))
    Z = np.empty((n, 3), order="F")
    K.precon_block(B, Z)
    assert np.isfinite(Z).all() and Z.any()
    assert live_bytes() - held == K.block_info()["bytes"]  # the block cycle's level vectors, where the mode has them
    K.close()
    returned(base)


# ------------------------------------------------------------------------------------------------ refused creations

def refused(create, exc, match):
    base = start()[0]
    with pytest.raises(exc, match=match):
        create()
    returned(base)


def test_a_refused_single_precision_range_returns_everything():
    """test_the_single_precision_range_galerkin: the rounding of a level, after the level vectors and the double level
    operators were allocated"""
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    S = varying_operator(grid, "smooth", 0.3)
    for scale in (1e39, 1e-40):
        T = S.copy()
        T.data = T.data * scale
        A = gk.device_csr_from(T)
        refused(lambda: dev.DeviceMultigrid32(A, grid, galerkin=True), ValueError, "single-precision range")
    T = S.copy()
    T.data = T.data * (3.0e38 / S.diagonal().max())  # the diagonal still fits, omega / diagonal falls below FLT_MIN
    A = gk.device_csr_from(T)
    refused(lambda: dev.DeviceMultigrid32(A, grid, omega=0.01, galerkin=True), ValueError, "single-precision range")


def test_a_refused_line_pivot_returns_everything():
    """test_a_failing_line_pivot_is_singular: the factorisation of the line operators, the last step of the creation"""
    from pysparse_amd import device as dev
    from pysparse_amd._capi import PspError
    grid, line = (5, 6), 1
    S = graded_operator(grid, line, 10.0)
    Cc = S.tocoo()
    along = np.abs(Cc.row - Cc.col) == 5
    bad = sp.coo_matrix((np.where(along, 3.0 * Cc.data, Cc.data), (Cc.row, Cc.col)), shape=S.shape).tocsr()
    bad.sort_indices()
    A = gk.device_csr_from(bad)
    refused(lambda: dev.DeviceMultigridLine(A, grid, line=line), PspError, "pivot")


def last_bit(S, row, col):
    """S with one direction of the pair (row, col) moved by one unit in the last place"""
    P = S.copy()
    k = P.indptr[row] + list(P.indices[P.indptr[row]:P.indptr[row + 1]]).index(col)
    P.data[k] = np.nextafter(P.data[k], 0.0)
    return P


def test_a_refused_unsymmetric_pair_returns_everything():
    """one unsymmetric pair each from test_refusals_name_their_reason (galerkin=True),
    test_refusals_from_the_device_pass_name_their_kind (stencil='box') and
    test_device_side_refusals_reach_the_caller_unchanged (interp='operator'): the checking pass, after the levels exist"""
    from pysparse_amd import device as dev
    grid = (9, 8, 7)
    A = gk.device_csr_from(last_bit(varying_operator(grid, "smooth", 0.3), 200, 201))
    refused(lambda: dev.DeviceMultigrid(A, grid, galerkin=True), ValueError, "unsymmetric")
    grid = (7, 12)
    A = gk.device_csr_from(last_bit(box_operator(grid, "q1kappa"), 30, 38))
    refused(lambda: dev.DeviceMultigridBox(A, grid), ValueError, "unsymmetric")
    grid = (9, 7)
    A = gk.device_csr_from(last_bit(interp_operator(grid, "b2_1e4"), 20, 21))
    refused(lambda: dev.DeviceMultigridInterp(A, grid), ValueError, "unsymmetric")
