"""Deep Jacobi-PCG / Jacobi-MINRES solves on an ill-conditioned irregular operator (BASELINE.json configs[4]'s
shape: an sss_mat with a scattered numbering).  The default stand-in converges in about 14 iterations; the conditioned
one (fem_sss_arrays(..., anisotropy=1e-4)) needs about 2000, so the fused loops on the stored numbering (csr_spmv_w5),
the permuted system behind the renumbered copy (csr_spmv_w3_rcm), a solve that crosses the copy's cost rule and the
stagnation exit all run at depth.  Every solve is compared with three CPU legs of the same k (tests/deep_krylov.py):
the oracle, the oracle on a permuted system, and the compiled reference kernels."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import deep_krylov as DK

pytestmark = pytest.mark.gpu

SOLVERS = ("pcg", "minres")
# converging solves: below 2048 products on a fresh handle (the copy's threshold), >= 1500 iterations
CONV_TOL = {"pcg": 1e-9, "minres": 1e-10}
STAG_TOL = 1e-15  # below what PCG can attain here: its stagnation exit (pcg.c) ends the solve
MAXIT = 4000
W2_VARIANT = 16578


def _row(case, kern, leg, sx, bar, dx, t):
    print("\n| %s | %s | %d (info %d) | %.1e | %.1e | %.1e | %.2f s |" % (case, kern, leg.iter, leg.info, sx, bar, dx, t))


@pytest.fixture(scope="module")
def mid(oracle):
    """the mid-size conditioned stand-in (n = 41 472) and every CPU leg the tests below compare against"""
    t0 = time.time()
    arrays, So, b, dinv = DK.standin(oracle)
    carrays, Sc, bc, dc = DK.standin(oracle, constant_diag=True)
    n = So.n
    perm = DK.seeded_perm(n, DK.LEG_SEED)
    A = oracle.sss_to_csr(So)
    Ap = DK.permuted_csr(oracle, A, perm)
    Ac = oracle.sss_to_csr(Sc)
    Acp = DK.permuted_csr(oracle, Ac, perm)
    jobs = {}
    for s in SOLVERS:
        for k in DK.DEPTHS:
            jobs.update(DK.leg_jobs(oracle, s, So, Ap, perm, b, dinv, 0.0, k, ("sss", s, k)))
        jobs.update(DK.leg_jobs(oracle, s, So, Ap, perm, b, dinv, CONV_TOL[s], MAXIT, ("sss", s, "conv")))
        jobs.update(DK.leg_jobs(oracle, s, A, Ap, perm, b, dinv, 0.0, 500, ("csr", s, 500)))
        jobs.update(DK.leg_jobs(oracle, s, A, Ap, perm, b, dinv, CONV_TOL[s], MAXIT, ("csr", s, "conv")))
        jobs.update(DK.leg_jobs(oracle, s, Sc, Acp, perm, bc, dc, 0.0, 100, ("const", s, 100)))
        jobs.update(DK.leg_jobs(oracle, s, Sc, Acp, perm, bc, dc, 1e-10, 500, ("const", s, "conv")))
    jobs.update(DK.leg_jobs(oracle, "pcg", So, Ap, perm, b, dinv, STAG_TOL, MAXIT, ("sss", "pcg", "stag")))
    res = DK.run_parallel(jobs)
    legs = {}
    for key, leg in res.items():
        legs.setdefault(key[:3], {})[key[3]] = leg
    print("\nCPU legs: %d solves in %.1f s" % (len(res), time.time() - t0))
    return {"arrays": arrays, "carrays": carrays, "So": So, "Sc": Sc, "A": A, "b": b, "bc": bc, "n": n, "legs": legs}


def _sss(arrays):
    from pysparse_amd import device as dev
    n, ind, col, val, diag = arrays
    return dev.DeviceSSS.from_arrays(n, ind, col, val, diag)


def _csr(A):
    from pysparse_amd import device as dev
    return dev.DeviceCSR.from_arrays(A.shape, A.ind, A.col, A.val)


def _solve(solver, H, b, tol, k):
    from pysparse_amd import device as dev
    x = np.zeros(H.shape[0])
    t = time.time()
    info, it, rr, h = getattr(dev, solver)(H, b, x, tol, k, dev.DeviceJacobi(H), hist=True)
    return DK.Leg(info, it, rr, x, h), time.time() - t


def _check(case, kern, got, t, legs, n, k, A=None, b=None):
    converged = got.info == 0
    bar, sx, dx = DK.compare(got, legs, n, k, A, b, converged=converged, history="minres" in case)
    assert sx <= DK.SPREAD_MAX, (case, sx)
    _row(case, kern, got, sx, bar, dx, t)


def _assert_w5(H):
    kern, info = H.kernel_info()
    assert kern == "csr_spmv_w5" and info["max_blocks"] > 64, (kern, info)
    assert H.setup_info()["reorder_state"] == -1


def _assert_rcm(H):
    kern, info = H.kernel_info()
    assert kern == "csr_spmv_w3_rcm" and info["max_blocks"] <= 64 < info["half_band"], (kern, info)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("form", ["sss", "csr"])
def test_stored_numbering_w5_at_depth(mid, solver, form):
    """(a, c) a fresh handle per solve multiplies on its stored numbering with csr_spmv_w5 (fused dot partials) for
    the whole solve: k = 100, 500, 1500 at tol = 0 and one converging solve, each under the 2048 products after which
    the cost rule would build the renumbered copy"""
    n, b, legs = mid["n"], mid["b"], mid["legs"]
    A = mid["So"] if form == "sss" else mid["A"]
    ks = DK.DEPTHS[:3] if form == "sss" else (500,)
    for k in ks + ("conv",):
        H = _sss(mid["arrays"]) if form == "sss" else _csr(mid["A"])
        _assert_w5(H)
        tol, maxit = (0.0, k) if k != "conv" else (CONV_TOL[solver], MAXIT)
        got, t = _solve(solver, H, b, tol, maxit)
        assert H.kernel_info()[0] == "csr_spmv_w5" and H.setup_info()["reorder_state"] == -1
        assert H.setup_info()["products_counted"] < 2048
        _check("%s %s w5 k=%s" % (form, solver, k), "csr_spmv_w5", got, t, legs[(form, solver, k)], n, maxit, A, b)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("form", ["sss", "csr"])
def test_permuted_system_at_depth(mid, solver, form):
    """(b, c) after prepare(1 << 30) the handle multiplies through the renumbered copy and the solvers run the permuted
    system (b, x0, dinv gathered once, x gathered back once): the same depths on one prepared handle"""
    n, b, legs = mid["n"], mid["b"], mid["legs"]
    A = mid["So"] if form == "sss" else mid["A"]
    H = _sss(mid["arrays"]) if form == "sss" else _csr(mid["A"])
    H.prepare(1 << 30)
    _assert_rcm(H)
    ks = DK.DEPTHS[:3] if form == "sss" else (500,)
    for k in ks + ("conv",):
        tol, maxit = (0.0, k) if k != "conv" else (CONV_TOL[solver], MAXIT)
        got, t = _solve(solver, H, b, tol, maxit)
        _check("%s %s rcm k=%s" % (form, solver, k), "csr_spmv_w3_rcm", got, t, legs[(form, solver, k)], n, maxit, A, b)
    assert H.setup_info()["reorder_state"] == 1


@pytest.mark.parametrize("solver", SOLVERS)
def test_gather_variant_at_depth(mid, solver):
    """(d) the gather kernel (variant 16578, csr_spmv_w2) on the full mirror at k = 500"""
    H = _csr(mid["A"])
    H.set_variant(W2_VARIANT)
    assert H.kernel_info()[0] == "csr_spmv_w2"
    got, t = _solve(solver, H, mid["b"], 0.0, 500)
    _check("csr %s w2 k=500" % solver, "csr_spmv_w2", got, t, mid["legs"][("csr", solver, 500)], mid["n"], 500)


@pytest.mark.parametrize("solver", SOLVERS)
def test_constant_diagonal_through_the_permuted_system(mid, solver):
    """(e) a constant diagonal: dinv is a constant vector, which the permuted system registers as one in the copy's
    numbering (the vector kernels then skip the dinv stream) -- k = 100 at tol = 0 and a converging solve"""
    H = _sss(mid["carrays"])
    H.prepare(1 << 30)
    _assert_rcm(H)
    for k in (100, "conv"):
        tol, maxit = (0.0, k) if k != "conv" else (1e-10, 500)
        got, t = _solve(solver, H, mid["bc"], tol, maxit)
        _check("const %s rcm k=%s" % (solver, k), "csr_spmv_w3_rcm", got, t, mid["legs"][("const", solver, k)],
               mid["n"], maxit, mid["Sc"], mid["bc"])


def test_stagnation_exit_at_depth(mid):
    """(h) PCG to a tol below its attainable accuracy ends on its stagnation exit (info -5, pcg.c) at an iteration
    inside the CPU legs' range; on the permuted system, so that no crossing is involved"""
    H = _sss(mid["arrays"])
    H.prepare(1 << 30)
    got, t = _solve("pcg", H, mid["b"], STAG_TOL, MAXIT)
    legs = mid["legs"][("sss", "pcg", "stag")]
    assert all(leg.info == -5 for leg in legs.values()), legs
    _check("sss pcg rcm tol=%g" % STAG_TOL, "csr_spmv_w3_rcm", got, t, legs, mid["n"], MAXIT, mid["So"], mid["b"])


@pytest.mark.parametrize("solver", SOLVERS)
def test_crossing_the_cost_rule_at_the_default_threshold(mid, solver):
    """(f) a fresh handle solves to k = 2300 at tol = 0: it crosses the 2048 products after which the cost rule builds
    the renumbered copy.  The counters say so; a second fresh handle making the same calls returns the same bits; the
    next solve on the crossed handle has the bits of the same solve on a handle prepared from the start; the crossing
    solve meets the comparator against the CPU legs at k = 2300."""
    n, b, k = mid["n"], mid["b"], 2300
    H1 = _sss(mid["arrays"])
    _assert_w5(H1)
    got, t = _solve(solver, H1, b, 0.0, k)
    info = H1.setup_info()
    assert info["products_counted"] == 2048 and info["reorder_state"] == 1, info
    assert H1.kernel_info()[0] == "csr_spmv_w3_rcm"
    H2 = _sss(mid["arrays"])
    again, _ = _solve(solver, H2, b, 0.0, k)
    assert (again.info, again.iter, again.relres) == (got.info, got.iter, got.relres)
    assert np.array_equal(again.x, got.x) and np.array_equal(again.hist, got.hist, equal_nan=True)
    _check("sss %s crossing k=%d" % (solver, k), "w5 -> w3_rcm", got, t, mid["legs"][("sss", solver, k)], n, k,
           mid["So"], b)
    nxt, _ = _solve(solver, H1, b, 0.0, 500)
    H3 = _sss(mid["arrays"])
    H3.prepare(1 << 30)
    ref, _ = _solve(solver, H3, b, 0.0, 500)
    assert (nxt.info, nxt.iter, nxt.relres) == (ref.info, ref.iter, ref.relres)
    assert np.array_equal(nxt.x, ref.x) and np.array_equal(nxt.hist, ref.hist, equal_nan=True)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from pysparse_amd import device as dev
from pysparse_amd.tools.standins import fem_sss_arrays
from tests import deep_krylov as DK
n, ind, col, val, diag = fem_sss_arrays(*DK.MID, anisotropy=DK.ANISOTROPY)
b = np.random.default_rng(7).random(n)
out = {}
for s in ("pcg", "minres"):
    H = dev.DeviceSSS.from_arrays(n, ind, col, val, diag)
    x = np.zeros(n)
    info, it, rr, h = getattr(dev, s)(H, b, x, 0.0, 500, dev.DeviceJacobi(H), hist=True)
    si = H.setup_info()
    out[s + "_x"], out[s + "_hist"] = x, h
    out[s + "_res"] = np.array([info, it, rr])
    out[s + "_counters"] = np.array([si["products_counted"], si["reorder_state"], si["reorder_after"]])
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("after", [288, 289, 296, 300, 305])
def test_crossing_the_cost_rule_at_shallow_depth(mid, tmp_path, after):
    """(g) a child process with PSP_SPMV_REORDER_AFTER moved to a few thresholds around 300 products (the MINRES loop
    enqueues 16 iterations per read of its state: 288 / 304 and 289 / 305 are batch edges whether or not the first
    residual's product is counted, 296 and 300 lie inside a batch) solves to k = 500 on fresh handles: the crossing
    lands inside the running loop and the result meets the comparator against the CPU legs of k = 500"""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, PSP_TUNING="1", PSP_SPMV_REORDER_AFTER=str(after))
    code = _CHILD % DK.ROOT
    t = time.time()
    subprocess.run([sys.executable, "-c", code, out], env=env, check=True, timeout=180)
    t = time.time() - t
    r = np.load(out)
    for s in SOLVERS:
        products, state, thr = r[s + "_counters"]
        assert (products, state, thr) == (after, 1, after), (s, r[s + "_counters"])
        info, it, rr = r[s + "_res"]
        got = DK.Leg(info, it, rr, r[s + "_x"], r[s + "_hist"])
        _check("sss %s crossing at %d, k=500" % (s, after), "w5 -> w3_rcm", got, t / 2, mid["legs"][("sss", s, 500)],
               mid["n"], 500)


def test_configs4_size_against_the_compiled_reference(oracle):
    """the conditioned stand-in at configs[4]'s size (n = 929 424), k = 500 at tol = 0 on the default path (a fresh
    handle: csr_spmv_w5) and on the prepared one, against the compiled reference kernels only (an oracle leg would
    take minutes; the reference gets the row-parallel operator callbacks of the full mirror)"""
    import bench
    from pysparse_amd.tools.standins import fem_sss_arrays
    if not oracle.have_ref_krylov():
        pytest.skip("oracle/_ref was not built (needs the reference sources at build time)")
    k = 500
    t0 = time.time()
    arrays = fem_sss_arrays(68, 68, 67, 32, anisotropy=DK.ANISOTROPY)
    n, ind, col, val, diag = arrays
    So = oracle.SSS(n, val, diag, col, ind)
    A = oracle.sss_to_csr(So)
    b = np.random.default_rng(7).random(n)
    dinv = oracle.jacobi_dinv(diag)
    threads = max(1, bench._usable_cores() // 2)
    refs = DK.run_parallel({s: (lambda s=s: _ref_leg(oracle, s, A, b, dinv, k, threads)) for s in SOLVERS})
    print("\nconfigs[4] reference legs in %.1f s" % (time.time() - t0))
    bar = bench.parity_bound(n, k, "reference")
    for s in SOLVERS:
        ref = refs[s]
        for prepared in (False, True):
            H = _sss(arrays)
            if prepared:
                H.prepare(1 << 30)
            kern = H.kernel_info()[0]
            assert kern == ("csr_spmv_w3_rcm" if prepared else "csr_spmv_w5"), kern
            got, t = _solve(s, H, b, 0.0, k)
            if not prepared:
                assert H.setup_info()["reorder_state"] == -1
            assert (got.info, got.iter) == (ref.info, ref.iter), (s, got, ref)
            dx = DK.xdiff(got.x, ref.x)
            assert dx <= bar and DK.rdiff(got.relres, ref.relres) <= bar, (s, prepared, dx, got, ref, bar)
            _row("configs[4] %s %s k=%d" % (s, "rcm" if prepared else "w5", k), kern, got, float("nan"), bar, dx, t)


def _ref_leg(O, solver, A, b, dinv, k, threads):
    x = np.zeros(A.shape[0])
    info, it, rr, _ = O.ref_krylov(solver, A, b, x, 0.0, k, ("jacobi", dinv), threads=threads)
    return DK.Leg(info, it, rr, x)
