"""precon.multigrid(..., precision='single') without a GPU: the argument checks, the new symbols,
and the float32 NumPy leg -- the oracles of tests/test_multigrid_host.py and tests/test_multigrid_galerkin_host.py with
every level matrix, P, R, omega / diagonal and the coarsest inverse cast to float32, b cast at entry and the result
widened at exit.  tests/test_gpu_multigrid_single.py imports the leg and the case lists from here.

The guard.  The GPU test allows max(64 eps32, 8 e32) max|z_ref| with e32 this leg's own distance from the reference (the
extended cycle with stored level operators, the float64 oracle in the matrix-free mode).  The guard asserts
e32 <= 8 eps32 on every GPU case, so that the GPU bound is 64 eps32 everywhere and a bad reference leg can never widen it.
Why 8: the float32 cycle is a few dozen float32 operations per point on data rounded once, and the cycle contracts -- the
float64 oracles sit at 1 to 2 eps64 of the extended cycle on the same cases (section 9d), and the same arithmetic in float32
sits where they do in its own unit; measured, at most 5.9 eps32 (the 1-D grid (4100,) with rough kappa)."""
import functools
import inspect
import os

import numpy as np
import pytest

from test_multigrid_host import CycleOracle, numpy_pcg, oracle_for
from test_multigrid_galerkin_host import GalerkinOracle, galerkin_oracle_for

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

# the GPU cases (tests/test_gpu_multigrid_single.py runs exactly these)
G_GRIDS = [(7,), (64,), (4100,), (5, 4), (37, 50), (130, 67), (9, 8, 7), (16, 16, 3), (20, 24, 28), (33, 31, 35)]
G_KINDS = ("smooth", "rand1e4")
G_SHIFTS = (0.0, 0.3)
PARAMS = ((0.8, 2), (1.0, 1), (2.0 / 3.0, 3))
SEEDS = (0, 1)
SOLVER_GRIDS = [(37, 50), (20, 24, 28)]
SOLVER_KINDS = ("smooth", "inclusion1e4")


def mf_cases():
    """the matrix-free cases: tests/test_gpu_multigrid.py's, imported not copied (importing it touches no device)"""
    from test_gpu_multigrid import CASES, IDS
    return CASES, IDS


def gid(g):
    return "x".join(map(str, g))


def rhs(grid, seed=0):
    return np.random.default_rng(seed).standard_normal(int(np.prod(grid)))


# ------------------------------------------------------------------------------------------------ the float32 leg

class Single:
    """the float32 leg of a CycleOracle or a GalerkinOracle: its level matrices, P, R and the coarsest inverse cast to
    float32, omega / diagonal formed in float64 and cast; apply() casts b, runs the oracle's cycle in float32 and widens"""

    def __init__(self, oracle):
        assert isinstance(oracle, (CycleOracle, GalerkinOracle))
        self.o = oracle
        self.A = [M.astype(F32) for M in oracle.A]
        self.P = [M.astype(F32) for M in oracle.P]
        self.R = [M.astype(F32) for M in oracle.R]
        self.inv = oracle.inv.astype(F32)

    def w(self, level, omega):
        return np.asarray(omega / np.asarray(self.o.d[level], dtype=np.float64)).astype(F32)

    def _cycle(self, b, omega, steps, level):
        if level == len(self.o.grids) - 1:
            return self.inv @ b
        A, w = self.A[level], self.w(level, omega)
        x = np.zeros_like(b)
        for _ in range(steps):
            x = x + w * (b - A @ x)
        x = x + self.P[level] @ self._cycle(self.R[level] @ (b - A @ x), omega, steps, level + 1)
        for _ in range(steps):
            x = x + w * (b - A @ x)
        assert x.dtype == F32
        return x

    def apply(self, b, omega=0.8, steps=2):
        return self._cycle(np.asarray(b, dtype=np.float64).astype(F32), omega, steps, 0).astype(np.float64)


@functools.lru_cache(maxsize=None)
def single_galerkin(grid, kind, s=0.0):
    return Single(galerkin_oracle_for(tuple(grid), kind, s))


@functools.lru_cache(maxsize=None)
def single_mf(grid, c=None, s=0.0):
    return Single(oracle_for(tuple(grid), c, s))


def leg_distance(O, O32, b, omega, steps):
    """(z_ref, e32): the reference cycle -- extended where the oracle has one -- and the float32 leg's distance from it in
    units of max|z_ref|"""
    ref = O.apply_ext(b, omega, steps) if hasattr(O, "apply_ext") else O.apply(b, omega, steps)
    ref = np.asarray(ref)
    scale = float(np.abs(ref).max())
    e32 = float(np.abs(O32.apply(b, omega, steps) - ref).max()) / scale
    return ref, e32


@functools.lru_cache(maxsize=None)
def pcg_counts(mode, grid, kind_or_c, s=0.0):
    """(iterations with the float64 leg, with the float32 leg) of NumPy PCG to 1e-8 on the case's operator"""
    if mode == "galerkin":
        O, O32 = galerkin_oracle_for(grid, kind_or_c, s), single_galerkin(grid, kind_or_c, s)
    else:
        O, O32 = oracle_for(grid, kind_or_c, s), single_mf(grid, kind_or_c, s)
    b = rhs(grid, 11)
    return numpy_pcg(O.A[0], b, 1e-8, 200, O.apply)[1], numpy_pcg(O.A[0], b, 1e-8, 200, O32.apply)[1]


# the matrix-free twins of the solver cases: the same grids, the library's Poisson operator and a general c with a shift
MF_SOLVER_CASES = [((37, 50), None, 0.0), ((37, 50), (2.5, 0.7), 0.3), ((20, 24, 28), None, 0.0),
                   ((20, 24, 28), (4.0, 1.0, 0.5), 0.01)]


# ------------------------------------------------------------------------------------------------ arguments

def ll(n, m=None):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, m or n)
    for i in range(min(n, m or n)):
        A[i, i] = 2.0
    return A


def test_precision_is_a_keyword_and_documented():
    from pysparse.precon import precon
    assert "precision='double'" in precon.multigrid.__doc__ and "galerkin=False" in precon.multigrid.__doc__
    with pytest.raises(TypeError):  # not a sixth positional argument
        precon.multigrid(ll(6), (6,), 0.8, 2, False, "single")
    with pytest.raises(TypeError):
        precon.multigrid(ll(6), (6,), 0.8, 2, "single")


@pytest.mark.parametrize("bad", [1, None, b"single", np.float32], ids=["int", "None", "bytes", "dtype"])
def test_a_precision_that_is_no_str_is_a_type_error(bad):
    """(there is no device here: a call that reached the library would raise RuntimeError)"""
    from pysparse.precon import precon
    with pytest.raises(TypeError, match="precision"):
        precon.multigrid(ll(6), (6,), precision=bad)
    with pytest.raises(TypeError, match="precision"):
        precon.multigrid(ll(6), (7,), galerkin=True, precision=bad)  # before the grid is looked at


@pytest.mark.parametrize("bad", ["half", "float32"])
def test_an_unknown_precision_is_a_value_error(bad):
    from pysparse.precon import precon
    with pytest.raises(ValueError, match="precision"):
        precon.multigrid(ll(6), (6,), precision=bad)
    with pytest.raises(ValueError, match="precision"):
        precon.multigrid(ll(6), (6,), galerkin=True, precision=bad)


@pytest.mark.parametrize("galerkin", [False, True])
@pytest.mark.parametrize("good", ["double", "single"])
def test_valid_strings_pass_the_parser(good, galerkin):
    """what surfaces is the ValueError of the later check of the grid, which does not mention the keyword"""
    from pysparse.precon import precon
    with pytest.raises(ValueError, match="grid") as e:
        precon.multigrid(ll(6), (7,), galerkin=galerkin, precision=good)
    assert "precision" not in str(e.value)
    with pytest.raises(ValueError, match="omega"):
        precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2, precision=good)


def test_device_multigrid32():
    from pysparse_amd import device
    assert issubclass(device.DeviceMultigrid32, device.DeviceMultigrid)
    assert (inspect.signature(device.DeviceMultigrid32.__init__) == inspect.signature(device.DeviceMultigrid.__init__))
    p = inspect.signature(device.DeviceMultigrid32.__init__).parameters
    assert list(p)[1:] == ["A", "grid", "omega", "steps", "galerkin"]
    assert device.DeviceMultigrid._FLAGS == 0 and device.DeviceMultigrid32._FLAGS == device.PSP_MG_SINGLE == 2
    assert device.PSP_MG_GALERKIN == 1
    assert callable(device.DeviceMultigrid.bytes)

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing below may reach the library
            self._h = None
            self.shape = shape

    with pytest.raises(TypeError):
        device.DeviceMultigrid32(FakeCSR((6, 6)), 6)
    with pytest.raises(ValueError):
        device.DeviceMultigrid32(FakeCSR((6, 6)), (7,), galerkin=True)


NEW_SYMBOLS = ("psp_mg_create_csr_ex", "psp_mg_create_sss_ex", "psp_mg_precision", "psp_mg_bytes")


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
    assert "#define PSP_MG_GALERKIN 1" in header and "#define PSP_MG_SINGLE 2" in header


# ------------------------------------------------------------------------------------------------ the guard

def test_the_leg_is_float32():
    O32 = single_galerkin((9, 8, 7), "smooth", 0.3)
    assert all(M.dtype == F32 for M in O32.A + O32.P + O32.R) and O32.inv.dtype == F32
    assert O32.w(0, 0.8).dtype == F32 and O32.w(0, 0.8).shape == (9 * 8 * 7,)
    assert np.array_equal(O32.w(0, 0.8), (0.8 / O32.o.d[0]).astype(F32))
    M32 = single_mf((9, 8, 7))
    assert M32.w(0, 0.8).dtype == F32 and M32.w(0, 0.8) == F32(0.8 / 6.0)
    z = O32.apply(rhs((9, 8, 7)))
    assert z.dtype == np.float64 and np.array_equal(z, z.astype(F32).astype(np.float64))


@pytest.mark.parametrize("s", G_SHIFTS)
@pytest.mark.parametrize("kind", G_KINDS)
@pytest.mark.parametrize("grid", G_GRIDS, ids=gid)
def test_guard_galerkin(grid, kind, s):
    O, O32 = galerkin_oracle_for(grid, kind, s), single_galerkin(grid, kind, s)
    worst = 0.0
    for omega, steps in PARAMS:
        for seed in SEEDS:
            _, e32 = leg_distance(O, O32, rhs(grid, seed), omega, steps)
            worst = max(worst, e32)
            assert e32 <= 8.0 * EPS32, (grid, kind, s, omega, steps, seed, e32 / EPS32)
    print("galerkin %s %s s %.1f: the float32 leg is at most %.2f eps32 from the extended cycle" % (grid, kind, s, worst / EPS32))


@pytest.mark.parametrize("grid,c,s", mf_cases()[0], ids=mf_cases()[1])
def test_guard_matrix_free(grid, c, s):
    O, O32 = oracle_for(grid, c, s), single_mf(grid, c, s)
    worst = 0.0
    for omega, steps in PARAMS:
        for seed in SEEDS:
            _, e32 = leg_distance(O, O32, rhs(grid, seed), omega, steps)
            worst = max(worst, e32)
            assert e32 <= 8.0 * EPS32, (grid, c, s, omega, steps, seed, e32 / EPS32)
    print("matrix-free %s c %s s %s: the float32 leg is at most %.2f eps32 from the float64 oracle" % (grid, c, s, worst / EPS32))


# ------------------------------------------------------------------------------------------------ PCG counts

@pytest.mark.parametrize("kind", SOLVER_KINDS)
@pytest.mark.parametrize("grid", SOLVER_GRIDS, ids=gid)
def test_pcg_counts_galerkin(grid, kind):
    it64, it32 = pcg_counts("galerkin", grid, kind)
    print("galerkin %s %s: PCG to 1e-8 in %d iterations with the float64 leg, %d with the float32 leg" % (grid, kind, it64, it32))
    assert it32 == it64 and it64 < 200


@pytest.mark.parametrize("grid,c,s", MF_SOLVER_CASES)
def test_pcg_counts_matrix_free(grid, c, s):
    it64, it32 = pcg_counts("mf", grid, c, s)
    print("matrix-free %s c %s: PCG to 1e-8 in %d iterations with the float64 leg, %d with the float32 leg" % (grid, c, it64, it32))
    assert it32 == it64 and it64 < 200
