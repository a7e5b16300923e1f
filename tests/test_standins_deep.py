"""The ill-conditioned irregular stand-in (pysparse_amd/tools/standins.py, anisotropy=) and the comparator of the deep
GPU tests (tests/deep_krylov.py, used by tests/test_gpu_irregular_deep.py) on the CPU: the defaults of the generator
are unchanged to the bit, the conditioned form keeps the pattern, is SPD and needs the depth it was made for, and the
comparator accepts a solve that differs only in its summation order but rejects a wrong gather or a lost term."""
import hashlib

import numpy as np
import pytest

from tests import deep_krylov as DK


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# recorded from the generator before the anisotropy= / constant_diag= options were added
DEFAULT_SHA = {
    (): ("e3bdb54490c3829d5a679dd4e47300462491d62d2531830596411c1bb7679911",
         "970be9981853c7070ab9b48104befe4e71039b722b6bc16e222feba4faf76e29",
         "aa91cd85f4b2a05b26747691cd426701c30b7f0c95a54124225fb100018b16ba",
         "0c096452b91a62d333f54f639983eab86aeaab25cd03efd0623963a51e803a5a"),
    (0, 6): ("6d68933ba27ed341e5627366840148d3c327592ac27bc6f19c46c6bdc9b2ced7",
             "49f55a5fe4ac68efbf175305dde26a80baf4c2b521005ee2dc6b0252c6d98e0e",
             "f232ed667bced88b3d61e9f020063bac923e6c16e10c7e53cc5a4cedfc274bcd",
             "0c096452b91a62d333f54f639983eab86aeaab25cd03efd0623963a51e803a5a"),
}


@pytest.mark.parametrize("extra", sorted(DEFAULT_SHA))
def test_default_standin_unchanged(extra):
    """bench.py --mtx standin:* and the existing tests depend on the default output: not one bit of it may move"""
    from pysparse_amd.tools.standins import fem_sss_arrays
    n, ind, col, val, diag = fem_sss_arrays(20, 18, 16, 512, *extra)
    assert n == 17280
    assert (ind.dtype, col.dtype, val.dtype, diag.dtype) == (np.int32, np.int32, np.float64, np.float64)
    assert tuple(_sha(a) for a in (ind, col, val, diag)) == DEFAULT_SHA[extra]


def test_conditioned_standin_is_well_formed(oracle):
    """Same pattern as the default stand-in (so the same kernels are chosen), SPD by Gershgorin (a positive diagonal
    strictly above the off-diagonal row sums), a constant diagonal with constant_diag=True, and the depth it was made
    for: the oracle's Jacobi-PCG and Jacobi-MINRES need >= 1500 iterations to tol = 1e-10."""
    from pysparse_amd.tools.standins import fem_sss_arrays
    n, ind, col, val, diag = fem_sss_arrays(*DK.MID)
    for constant in (False, True):
        (n2, ind2, col2, val2, diag2), So, b, dinv = DK.standin(oracle, constant_diag=constant)
        assert n2 == n and np.array_equal(ind2, ind) and np.array_equal(col2, col)
        absum = np.bincount(np.repeat(np.arange(n), np.diff(ind)), np.abs(val2), minlength=n)
        absum += np.bincount(col2, np.abs(val2), minlength=n)
        assert np.all(diag2 > 0) and np.all(diag2 > absum)
        assert np.all(val2 < 0) and np.abs(val2).min() < 1e-3 * np.abs(val2).max()  # couplings of two strengths
        if constant:
            assert np.all(diag2 == diag2[0])
        else:
            assert np.ptp(diag2) > 0.1 * diag2.max()
    _, So, b, dinv = DK.standin(oracle)
    got = DK.run_parallel({s: (lambda s=s: DK.oracle_leg(oracle, s, So, b, dinv, 1e-10, 5000))
                           for s in ("pcg", "minres")})
    for s, leg in got.items():
        assert leg.info == 0 and leg.iter >= 1500, (s, leg)
    with pytest.raises(ValueError):
        fem_sss_arrays(4, 4, 4, 1, anisotropy=1.5)


@pytest.fixture(scope="module")
def mutants(oracle):
    """the CPU legs and the three mutants at every tol = 0 depth of the GPU tests, both solvers"""
    _, So, b, dinv = DK.standin(oracle)
    perm = DK.seeded_perm(So.n, DK.LEG_SEED)
    Ap = DK.permuted_csr(oracle, oracle.sss_to_csr(So), perm)
    jobs = {}
    for solver in ("pcg", "minres"):
        for k in DK.DEPTHS:
            jobs.update(DK.leg_jobs(oracle, solver, So, Ap, perm, b, dinv, 0.0, k, (solver, k)))
            jobs.update(DK.mutant_jobs(oracle, solver, So, b, dinv, k, (solver, k)))
    return So.n, DK.run_parallel(jobs)


@pytest.mark.parametrize("solver", ["pcg", "minres"])
@pytest.mark.parametrize("k", DK.DEPTHS)
def test_comparator_has_teeth(mutants, solver, k):
    """At every depth the GPU tests use, the legs agree in x to far better than SPREAD_MAX, and the comparator accepts
    the oracle in another summation order (c) but rejects one block of dinv in the wrong numbering (a) and one
    dropped stored entry (b).  (Past convergence (k = 2300) a wrong preconditioner leads to the same x; (a) is then
    caught by its residual norms.)"""
    n, res = mutants
    legs = {name: res[(solver, k, name)] for name in ("oracle", "permuted", "reference")}
    bar_x, _, sx = DK.bars(legs, n, k)
    assert sx <= DK.SPREAD_MAX, (solver, k, sx)
    DK.compare(res[(solver, k, "reordered")], legs, n, k, history=True)
    for name in ("dinv_block", "dropped"):
        with pytest.raises(AssertionError):
            DK.compare(res[(solver, k, name)], legs, n, k, history=True)
        if legs["reference"].relres > 1e-9:  # before convergence: rejected on x alone, not only on the residual norms
            assert DK.xdiff(res[(solver, k, name)].x, legs["reference"].x) > bar_x, (solver, k, name)
