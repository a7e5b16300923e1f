"""Deep Jacobi-PCG / Jacobi-MINRES solves on the ill-conditioned irregular stand-in, shared by
tests/test_standins_deep.py (CPU: the comparator rejects wrong solves) and tests/test_gpu_irregular_deep.py (GPU
against the CPU legs).

A solve is compared against three CPU legs that differ from each other only in the order of their sums:
  * "oracle"    -- the oracle's restatement (oracle.pcg / oracle.minres) on the SSS operator, with its history;
  * "permuted"  -- the oracle on P A P^T in CSR form for a seeded permutation P (b, dinv gathered, x gathered back);
  * "reference" -- the compiled reference kernels (oracle.ref_krylov) on the SSS operator.
The spread is the largest disagreement among them, taken apart for x and for the residual norms (see spreads); a
solve passes when it has the reference's info and an iteration count inside the legs' range (widened where the
legs disagree, see compare), lies within
bar = max(parity_bound(n, k, "reference"), 4 spread) of the reference in x and in relres (each with its own spread)
and of the oracle in its MINRES history, and, when it converged, has a true residual |b - A x| no larger than 10x the
reference's.  Plain NumPy and the oracle; nothing here touches the GPU."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (parity_bound, _usable_cores)
from pysparse_amd.tools.standins import fem_sss_arrays  # noqa: E402

MID = (24, 24, 24, 512)  # 41 472 rows: chunks reach > 64 x blocks (csr_spmv_w5), the copy qualifies (csr_spmv_w3_rcm)
ANISOTROPY = 1e-4
LEG_SEED = 1  # the permutation of the "permuted" leg
MUTANT_SEED = 2  # the permutation of mutant (c): another summation order than any leg's
SPREAD_MAX = 1e-6  # beyond this, rounding alone decides the iterates: the depth could not tell a bug from noise
DEPTHS = (100, 500, 1500, 2300)  # the tol = 0 depths of the GPU tests (2300: past the 2048 products of the cost rule)


def standin(O, grid=MID, constant_diag=False):
    """(arrays, So, b, dinv): fem_sss_arrays' (n, ind, col, val, diag) of the conditioned stand-in, the same as an
    oracle SSS, b = U(0, 1) (seeded: every mode of the operator present), Jacobi's dinv"""
    arrays = fem_sss_arrays(*grid, anisotropy=ANISOTROPY, constant_diag=constant_diag)
    n, ind, col, val, diag = arrays
    So = O.SSS(n, val, diag, col, ind)
    b = np.random.default_rng(7).random(n)
    return arrays, So, b, O.jacobi_dinv(diag)


def seeded_perm(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def permuted_csr(O, A, perm):
    """P A P^T in CSR form (sorted columns), row i of it = row perm[i] of A; A is a CSR"""
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.ind))
    r, c = inv[rows], inv[A.col.astype(np.int64)]
    order = np.lexsort((c, r))
    ind = np.zeros(A.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=ind[1:])
    return O.CSR(A.shape, A.val[order], c[order].astype(np.int32), ind)


class Leg:
    """what one solve returned: info, iter, relres, x, and (oracle legs) the residual history"""

    def __init__(self, info, it, relres, x, hist=None):
        self.info, self.iter, self.relres, self.x, self.hist = int(info), int(it), float(relres), x, hist

    def __repr__(self):
        return "Leg(info=%d, iter=%d, relres=%.6e)" % (self.info, self.iter, self.relres)


def oracle_leg(O, solver, A, b, dinv, tol, k):
    x = np.zeros(A.shape[0])
    info, it, rr, h = getattr(O, solver)(A, b, x, tol, k, dinv, hist=True)
    return Leg(info, it, rr, x, h)


def permuted_leg(O, solver, Ap, perm, b, dinv, tol, k):
    """the oracle on the permuted system (Ap = P A P^T), x gathered back into A's numbering"""
    xp = np.zeros(Ap.shape[0])
    info, it, rr, h = getattr(O, solver)(Ap, np.ascontiguousarray(b[perm]), xp, tol, k,
                                         np.ascontiguousarray(dinv[perm]), hist=True)
    x = np.empty_like(xp)
    x[perm] = xp
    return Leg(info, it, rr, x, h)


def reference_leg(O, solver, A, b, dinv, tol, k):
    x = np.zeros(A.shape[0])
    info, it, rr, _ = O.ref_krylov(solver, A, b, x, tol, k, ("jacobi", dinv))
    return Leg(info, it, rr, x)


def run_parallel(jobs):
    """{key: fn()} for {key: fn}; the oracle's C calls release the GIL, so the legs run side by side"""
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), bench._usable_cores()))) as ex:
        futs = {key: ex.submit(fn) for key, fn in jobs.items()}
        return {key: f.result() for key, f in futs.items()}


def leg_jobs(O, solver, A, Ap, perm, b, dinv, tol, k, tag=()):
    """the three CPU legs of one solve as jobs for run_parallel, keyed tag + (leg name,)"""
    return {tag + ("oracle",): lambda: oracle_leg(O, solver, A, b, dinv, tol, k),
            tag + ("permuted",): lambda: permuted_leg(O, solver, Ap, perm, b, dinv, tol, k),
            tag + ("reference",): lambda: reference_leg(O, solver, A, b, dinv, tol, k)}


def mutant_jobs(O, solver, So, b, dinv, k, tag=()):
    """three wrong or re-ordered versions of the reference solve at depth k, as jobs for run_parallel:
      "dinv_block"  (a) one aligned 1024-row block of dinv taken in another numbering (a wrong gather of the permuted
                    system);
      "dropped"     (b) one stored lower-triangle entry dropped (a csr_spmv_w5 chunk that loses a term);
      "reordered"   (c) the oracle on P A P^T for another seeded P, permuted back: only the summation order changed."""
    n = So.n
    perm = seeded_perm(n, MUTANT_SEED)
    lo = 1024 * (n // 2048)
    dm = dinv.copy()
    dm[lo:lo + 1024] = dinv[perm[lo:lo + 1024]]
    vm = So.val.copy()
    vm[So.ind[n // 2 + 1] - 1] = 0.0  # the last stored entry of row n / 2
    Sm = type(So)(n, vm, So.diag, So.col, So.ind)
    Ap = permuted_csr(O, O.sss_to_csr(So), perm)
    return {tag + ("dinv_block",): lambda: oracle_leg(O, solver, So, b, dm, 0.0, k),
            tag + ("dropped",): lambda: oracle_leg(O, solver, Sm, b, dinv, 0.0, k),
            tag + ("reordered",): lambda: permuted_leg(O, solver, Ap, perm, b, dinv, 0.0, k)}


def xdiff(x, y):
    """max-norm relative difference of two iterates"""
    return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))


def rdiff(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def hdiff(h, g):
    """largest relative difference of two residual histories over the entries both wrote"""
    m = np.isfinite(h) & np.isfinite(g)
    if not m.any():
        return 0.0
    return float((np.abs(h[m] - g[m]) / np.maximum(np.abs(g[m]), 1e-300)).max())


def spreads(legs):
    """(x spread, residual spread): the largest CPU-vs-CPU disagreement among the legs {name: Leg} in x, and in relres
    and the residual histories (oracle legs).  They are kept apart because they behave differently at depth: once the
    Lanczos vectors lose orthogonality (here from about k = 1000 on) rounding delays convergence by a few iterations,
    which moves the residual norm at a given k by up to tens of percent while x stays within 1e-8."""
    names = sorted(legs)
    sx = sr = 0.0
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            sx = max(sx, xdiff(legs[p].x, legs[q].x))
            sr = max(sr, rdiff(legs[p].relres, legs[q].relres))
            if legs[p].hist is not None and legs[q].hist is not None:
                sr = max(sr, hdiff(legs[p].hist, legs[q].hist))
    return sx, sr


def true_residual(A, b, x):
    """|b - A x| on the host in long double (A: oracle SSS or CSR)"""
    xl, bl = x.astype(np.longdouble), b.astype(np.longdouble)
    if hasattr(A, "diag"):  # SSS: the diagonal, the stored lower triangle and its mirror
        rows = np.repeat(np.arange(A.n), np.diff(A.ind))
        v = A.val.astype(np.longdouble)
        y = A.diag.astype(np.longdouble) * xl
        np.add.at(y, rows, v * xl[A.col])
        np.add.at(y, A.col, v * xl[rows])
    else:
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.ind))
        y = np.zeros(A.shape[0], dtype=np.longdouble)
        np.add.at(y, rows, A.val.astype(np.longdouble) * xl[A.col])
    r = bl - y
    return float(np.sqrt(np.sum(r * r)))


def bars(legs, n, k):
    """(bar for x, bar for relres / history, x spread): max(parity_bound(n, k, "reference"), 4 spread) of each"""
    sx, sr = spreads(legs)
    pb = bench.parity_bound(n, k, "reference")
    return max(pb, 4.0 * sx), max(pb, 4.0 * sr), sx


def compare(got, legs, n, k, A=None, b=None, converged=False, history=False):
    """Check one solve `got` (a Leg) against the CPU legs of the same maxit k.  Returns (x bar, x spread, x difference
    to the reference); raises AssertionError naming what failed.  A, b: the operator and right-hand side, needed for
    the true-residual check of a converged solve; history: compare got.hist with the oracle's (MINRES)."""
    ref = legs["reference"]
    k = min(k, max(leg.iter for leg in legs.values()))  # a solve that ended early is as deep as it went
    bar_x, bar_r, sx = bars(legs, n, k)
    infos = sorted({leg.info for leg in legs.values()})
    its = sorted(leg.iter for leg in legs.values())
    if len(infos) == 1:
        assert got.info == ref.info, ("info", got, legs)
    else:
        assert got.info in infos, ("info outside the legs'", got, legs)
    if its[0] == its[-1]:
        assert got.iter == ref.iter, ("iter", got, legs)
    else:
        # where a solve exits at depth (convergence near tol = 1e-9, stagnation) its residual falls by about 1 % per
        # iteration, so rounding alone moves the exit by tens of iterations: the compiled reference's own exit moved by
        # 1.7 % between two x86 hosts (OpenBLAS picks its dot kernel by CPU).  The legs' range, widened by its width or
        # 2 % of the depth, whichever is larger.
        slack = max(its[-1] - its[0], int(0.02 * its[-1]))
        assert its[0] - slack <= got.iter <= its[-1] + slack, ("iter outside the legs' range", got, legs)
    dx = xdiff(got.x, ref.x)
    assert dx <= bar_x, ("x", dx, bar_x, got, legs)
    dr = rdiff(got.relres, ref.relres)
    assert dr <= bar_r, ("relres", got.relres, ref.relres, bar_r)
    if history:
        dh = hdiff(got.hist, legs["oracle"].hist)
        assert dh <= bar_r, ("history", dh, bar_r)
    if converged:
        tr, tr_ref = true_residual(A, b, got.x), true_residual(A, b, ref.x)
        assert tr <= 10.0 * tr_ref, ("true residual", tr, tr_ref)
    return bar_x, sx, dx
