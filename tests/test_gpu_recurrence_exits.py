"""GPU: the breakdown exits of the scalar recurrences (pysparse_amd/csrc/psp_recur.h) on every route that evaluates them.

The operator is diag(+1, -1, +1, ...): symmetric, indefinite, and built so that the first dot product of a solve
vanishes.  With b = ones PCG meets p.q = 0 in iteration 1 (pcg.c:118-120, info -6) and, with Jacobi, rho = r.z = 0
(pcg.c:101-104, info -2); qmrs leaves through its eps0 / delta tests with the same codes.  The suite reaches these
exits otherwise only through zero right-hand sides.  Every sum here adds small integers, so the expected values are
exact in any summation order: the answers must EQUAL the oracle's (oracle/pysparse_oracle.c on the CPU), which are
    pcg  / none   -> (-6, 1, 1.0), x = 0        pcg  / jacobi -> (-2, 1, 1.0), x = 0
    qmrs / none   -> (-6, 1, 1.0)               qmrs / jacobi -> (-2, 1, 1.0)
    pcg with b = 0, x0 = ones -> (0, 0, 0.0), x = 0
on each route: the default one (at n = 4096 the single-kernel loop of psp_coop.hip), PSP_COOP=0 (a launch per phase,
scalars on the device: the lazy PCG loop), PSP_COOP=0 PSP_PCG_ASYNC=0 PSP_KRY_DEVSCAL=0 (scalars on the host), and
PSP_COOP=0 PSP_MID=0 PSP_PCG_LAZYX=0 (the eager PCG loop with device scalars, at n = 32768 too); and, in each of them,
from the batched PCG with k = 2: the breaking column b = ones beside a healthy one, which must still converge.

The healthy column: b = A e with e = 1 on the rows whose diagonal entry is +1 and 0 elsewhere (so b = e, and PCG
converges in one iteration to x = e).  b = A ones itself is NOT healthy on this operator -- p = b gives
p.q = sum(+1, -1, ...) = 0, the oracle returns -6 for it too -- so the test pins that column as a second breaking one.

MINRES, cgs and bicgstab are left out on purpose: on this operator the reference itself returns NaN for them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_BIG = 4096, 32768
TOL, MAXIT = 1e-8, 50

ROUTES = {
    "default": {},
    "launch_per_phase_device_scalars": {"PSP_COOP": "0"},
    "launch_per_phase_host_scalars": {"PSP_COOP": "0", "PSP_PCG_ASYNC": "0", "PSP_KRY_DEVSCAL": "0"},
    # the eager device-scalar PCG loop at both sizes (the default below 2^24 rows is the lazy one; PSP_MID=0: not pcg_mid)
    "launch_per_phase_eager_pcg": {"PSP_COOP": "0", "PSP_MID": "0", "PSP_PCG_LAZYX": "0"},
}

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from pysparse_amd import device as dev

def diag_pm(n):
    ind = np.arange(n + 1, dtype=np.int32)
    col = np.arange(n, dtype=np.int32)
    val = np.where(np.arange(n) %% 2 == 0, 1.0, -1.0)
    return dev.DeviceCSR.from_arrays((n, n), ind, col, val), val

tol, maxit = %(tol)r, %(maxit)d
out = {}
for n in (%(n)d, %(n_big)d):
    D, d = diag_pm(n)
    x = np.zeros(n)
    r = dev.pcg(D, np.ones(n), x, tol, maxit)
    out["pcg_none_%%d" %% n] = [list(r), float(np.abs(x).max()), dev.last_solve_info()[0]]
n = %(n)d
D, d = diag_pm(n)
K = dev.DeviceJacobi(D)
x = np.zeros(n)
r = dev.pcg(D, np.ones(n), x, tol, maxit, K)
out["pcg_jacobi"] = [list(r), float(np.abs(x).max()), dev.last_solve_info()[0]]
for name, k in (("qmrs_none", None), ("qmrs_jacobi", K)):
    out[name] = [list(dev.qmrs(D, np.ones(n), np.zeros(n), tol, maxit, k))]
x = np.ones(n)
r = dev.pcg(D, np.zeros(n), x, tol, maxit)
out["pcg_zero_rhs"] = [list(r), float(np.abs(x).max())]
e = (d > 0).astype(np.float64)
for name, k in (("batch_none", None), ("batch_jacobi", K)):
    for tag, cols in (("", (np.ones(n), e)), ("_both_break", (np.ones(n), d * np.ones(n)))):
        B = np.column_stack(cols)
        X = np.zeros((n, 2))
        info, it, rr = dev.pcg_batch(D, B, X, tol, maxit, k)
        out[name + tag] = [[[int(info[c]), int(it[c]), float(rr[c])] for c in range(2)],
                           [float(np.abs(X[:, 0]).max()), float(np.abs(X[:, 1] - e).max())]]
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def expected(oracle):
    """The oracle's answers, computed once."""
    def diag_pm(n):
        val = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        return oracle.CSR((n, n), val, np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32)), val

    exp = {}
    for n in (N, N_BIG):
        A, d = diag_pm(n)
        x = np.zeros(n)
        exp["pcg_none_%d" % n] = (oracle.pcg(A, np.ones(n), x, TOL, MAXIT), x)
    A, d = diag_pm(N)
    dinv = oracle.jacobi_dinv(A.diagonal())
    x = np.zeros(N)
    exp["pcg_jacobi"] = (oracle.pcg(A, np.ones(N), x, TOL, MAXIT, dinv), x)
    exp["qmrs_none"] = (oracle.krylov_more("qmrs", A, np.ones(N), np.zeros(N), TOL, MAXIT), None)
    exp["qmrs_jacobi"] = (oracle.krylov_more("qmrs", A, np.ones(N), np.zeros(N), TOL, MAXIT, dinv), None)
    x = np.ones(N)
    exp["pcg_zero_rhs"] = (oracle.pcg(A, np.zeros(N), x, TOL, MAXIT), x)
    e = (d > 0).astype(np.float64)
    for name, k in (("none", None), ("jacobi", dinv)):
        for tag, b in (("healthy", e), ("a_ones", d * np.ones(N))):
            x = np.zeros(N)
            exp["col_%s_%s" % (tag, name)] = (oracle.pcg(A, b, x, TOL, MAXIT, k), x)
    # what the issue's table says the oracle returns; anything else means the fixture itself is wrong
    assert exp["pcg_none_%d" % N][0] == (-6, 1, 1.0) and exp["pcg_none_%d" % N_BIG][0] == (-6, 1, 1.0)
    assert exp["pcg_jacobi"][0] == (-2, 1, 1.0)
    assert exp["qmrs_none"][0] == (-6, 1, 1.0) and exp["qmrs_jacobi"][0] == (-2, 1, 1.0)
    assert exp["pcg_zero_rhs"][0] == (0, 0, 0.0)
    for key in ("pcg_none_%d" % N, "pcg_none_%d" % N_BIG, "pcg_jacobi", "pcg_zero_rhs"):
        assert not exp[key][1].any()
    for name in ("none", "jacobi"):
        assert exp["col_healthy_" + name][0][0] == 0 and np.array_equal(exp["col_healthy_" + name][1], e)
        assert exp["col_a_ones_" + name][0][0] in (-2, -6)
    return exp


@pytest.mark.parametrize("route", list(ROUTES))
def test_breakdown_exits_match_the_oracle(route, expected, record_property):
    env = dict(os.environ, PSP_TUNING="1")  # the master switch that makes the library read its A/B variables
    env.update(ROUTES[route])
    code = CHILD % {"root": ROOT, "tol": TOL, "maxit": MAXIT, "n": N, "n_big": N_BIG}
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    for key in ("pcg_none_%d" % N, "pcg_none_%d" % N_BIG, "pcg_jacobi"):
        record_property(route + ":" + key, got[key][2])  # which loop took it (recorded, not asserted)
        print(route, key, got[key])
    for key in ("pcg_none_%d" % N, "pcg_none_%d" % N_BIG, "pcg_jacobi", "pcg_zero_rhs"):
        assert tuple(got[key][0]) == expected[key][0], (route, key, got[key])
        assert got[key][1] == 0.0, (route, key, "x must be all zero")
    for key in ("qmrs_none", "qmrs_jacobi"):
        assert tuple(got[key][0]) == expected[key][0], (route, key, got[key])
    for name in ("none", "jacobi"):
        breaking = expected["pcg_none_%d" % N if name == "none" else "pcg_jacobi"][0]
        cols, (x0_max, x1_err) = got["batch_" + name]
        assert tuple(cols[0]) == breaking and x0_max == 0.0, (route, name, cols)
        assert tuple(cols[1]) == expected["col_healthy_" + name][0] and cols[1][0] == 0, (route, name, cols)
        assert x1_err == 0.0, (route, name, "the healthy column converges to e")
        cols, (x0_max, _) = got["batch_" + name + "_both_break"]
        assert tuple(cols[0]) == breaking and x0_max == 0.0, (route, name, cols)
        assert tuple(cols[1]) == expected["col_a_ones_" + name][0], (route, name, cols)
