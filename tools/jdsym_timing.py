"""Timing of the Jacobi-Davidson pieces (pysparse_amd/csrc/psp_bvec.hip, psp_jdsym.hip) -> profiles/jdsym_timing.json.

1. Kernels.  psp_bv_tdot / psp_bv_gemv / psp_bv_rotate at n = 2^24, m = 8, 16, 32: milliseconds (median of windows of
   device-event timed launches after a warm-up), model bytes over time, the same process's psp_stream_probe with a
   matching stream count as the ceiling, and the vector-at-a-time equivalent beside it (psp_k_dot x m for tdot,
   psp_k_x_update -- x += alpha p -- x m for gemv).
2. End to end.  jdsym (kmax 5, tau 0, qmrs, Jacobi) on poisson_csr(512, 512) and the fem32 stand-in against a host-loop
   baseline: the same algorithm in NumPy block algebra over what the package offered before (A.matvec, K.precon and
   krylov.qmrs with Python callbacks).  Wall time, outer and inner iterations of both; the baseline stops at a wall-time
   budget and reports how far it got.

    python tools/jdsym_timing.py [--out profiles/jdsym_timing.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(L, fn, reps, windows=5, warmup=3):
    """median over `windows` of (device time of `reps` calls of fn) / reps"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    L.psp_event_create(C.byref(e0))
    L.psp_event_create(C.byref(e1))
    for _ in range(warmup):
        fn()
    L.psp_synchronize()
    out = []
    for _ in range(windows):
        L.psp_event_record(e0)
        for _ in range(reps):
            fn()
        L.psp_event_record(e1)
        ms = C.c_float()
        L.psp_event_elapsed_ms(e0, e1, C.byref(ms))
        out.append(ms.value / reps)
    L.psp_event_destroy(e0)
    L.psp_event_destroy(e1)
    return statistics.median(out), min(out), max(out)


def probe(L, reads, writes, nbytes):
    avg, mn = C.c_float(), C.c_float()
    rc = L.psp_stream_probe(reads, writes, nbytes, 10, C.byref(avg), C.byref(mn))
    if rc != 0:
        return None
    return (reads + writes) * nbytes / (mn.value * 1e-3) / 1e9


def kernels(L, dev, n, ms_list):
    rows = []
    rng = np.random.default_rng(0)
    mmax = max(ms_list)
    dV = dev.DeviceBuffer(n * mmax)
    chunk = rng.standard_normal(n)
    for c in range(mmax):  # the same column everywhere: the values do not matter for the time
        L.psp_memcpy_h2d(dV.ptr + 8 * n * c, chunk.ctypes.data, 8 * n)
    dx, dy = dev.DeviceBuffer.from_host(chunk), dev.DeviceBuffer.from_host(chunk)
    dh = dev.DeviceBuffer.from_host(np.full(mmax + 8, 1e-3))
    dout = dev.DeviceBuffer(16)
    for m in ms_list:
        U = np.ascontiguousarray(rng.standard_normal((m, m)))
        jn = m // 2
        cases = [
            ("tdot", lambda: L.psp_bv_tdot(n, m, dV.ptr, n, dx.ptr, dh.ptr), 8 * n * (m + 1), (min(8, m + 1), 0),
             ("psp_k_dot x m", lambda: [L.psp_k_dot(n, dV.ptr + 8 * n * c, dx.ptr, dout.ptr) for c in range(m)], 16 * n * m)),
            ("gemv", lambda: L.psp_bv_gemv(n, m, dV.ptr, n, dh.ptr, -1.0, 1.0, dy.ptr), 8 * n * (m + 2), (min(8, m + 1), 1),
             ("psp_k_x_update x m", lambda: [L.psp_k_x_update(n, 1e-3, dV.ptr + 8 * n * c, dy.ptr, dout.ptr) for c in range(m)],
              24 * n * m)),
            ("rotate", lambda: L.psp_bv_rotate(n, m, dV.ptr, n, U.ctypes.data, m, 0, jn, 0), 8 * n * (m + jn), (8, 1), None),
        ]
        for name, fn, model, (rd, wr), other in cases:
            med, lo, hi = event_ms(L, fn, reps=5)
            ceiling = probe(L, rd, wr, 8 * n)
            row = {"kernel": name, "n": n, "m": m, "ms_median": med, "ms_min": lo, "ms_max": hi, "model_bytes": model,
                   "model_GBps": model / (med * 1e-3) / 1e9, "probe_streams": [rd, wr], "probe_GBps": ceiling}
            if name == "rotate":
                row["jn"] = jn
                # every call uploads its U (pageable host memory) and waits for that copy before it launches: the window
                # between the events holds those host stalls too, so this is the time of the call, not of the kernel
                row["ms_is"] = "whole call: upload of U + wait + kernel"
            if other:
                oname, ofn, obytes = other
                omed, olo, ohi = event_ms(L, ofn, reps=2)
                row["vector_at_a_time"] = {"what": oname, "ms_median": omed, "bytes": obytes, "speedup": omed / med}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


# ---------------------------------------------------------------------- host-loop baseline

def host_jdsym(A, K, n, kmax, tau, jdtol, itmax, qmrs, jmax=25, jmin=10, linitmax=200, eps_tr=1e-3, toldecay=1.5,
               budget_s=120.0, seed=0):
    """Jacobi-Davidson (blksize 1, no mass matrix, symmetric operator type) with NumPy block algebra on the host; the
    products, the preconditioner and the inner solver are the package's public calls"""
    t0 = time.perf_counter()
    rng = np.random.default_rng(seed)

    def mv(x):
        y = np.empty(n)
        A.matvec(np.ascontiguousarray(x), y)
        return y

    def prec(x):
        y = np.empty(n)
        K.precon(np.ascontiguousarray(x), y)
        return y

    Q, Y = np.zeros((n, kmax)), np.zeros((n, kmax))
    H = np.zeros((kmax, kmax))
    lam = []
    V = np.zeros((n, jmax))
    v = rng.random(n)
    V[:, 0] = v / np.linalg.norm(v)
    j, k, it, inner, step = 1, 0, 0, 0, 1
    Mh = np.zeros((jmax, jmax))
    Mh[0, 0] = V[:, 0] @ mv(V[:, 0])

    class CorrEq(object):
        shape = (n, n)

        def __init__(self, kk, theta):
            self.Q, self.Y, self.kk, self.theta = Q[:, :kk], Y[:, :kk], kk, theta
            self.Hinv = np.linalg.inv(H[:kk, :kk])

        def matvec(self, x, y):
            w = mv(x) - self.theta * x
            y[:] = w - self.Q @ (self.Q.T @ w)

        def precon(self, x, y):
            w = prec(x)
            y[:] = w - self.Y @ (self.Hinv @ (self.Q.T @ w))

    timed_out = False
    while it < itmax and k < kmax:
        s, U = np.linalg.eigh(Mh[:j, :j])
        order = np.argsort(np.abs(s - tau), kind="stable")
        s, U = s[order], U[:, order]
        while True:
            q = V[:, :j] @ U[:, 0]
            r = mv(q) - s[0] * q
            Q[:, k] = q
            Y[:, k] = prec(q)
            H[:k + 1, k] = Q[:, :k + 1].T @ Y[:, k]
            H[k, :k + 1] = Y[:, :k + 1].T @ q
            resnrm = np.linalg.norm(r)
            found = resnrm < jdtol and (j > 1 or k == kmax - 1)
            if found:
                lam.append(s[0])
                V[:, :j - 1] = V[:, :j] @ U[:, 1:j]
                s, j, k, step = s[1:], j - 1, k + 1, 1
                Mh[:, :] = 0.0
                Mh[:j, :j] = np.diag(s[:j])
                U = np.eye(j)
                if k == kmax:
                    break
            if j + 1 > jmax:
                V[:, :jmin] = V[:, :j] @ U[:, :jmin]
                j = jmin
                Mh[:, :] = 0.0
                Mh[:j, :j] = np.diag(s[:j])
                U = np.eye(j)
            if not found:
                break
        if k == kmax:
            break
        ce = CorrEq(k + 1, s[0] if resnrm < eps_tr else tau)
        r = r - ce.Q @ (ce.Q.T @ r)
        x = np.zeros(n)
        info, linit, relres = qmrs(ce, r, x, toldecay ** (-step), linitmax, ce)
        step += 1
        inner += linit
        for i in range(k + 1):
            x -= Q[:, i] * (Q[:, i] @ x)
        nrm = np.linalg.norm(x)
        for _ in range(5):
            x -= V[:, :j] @ (V[:, :j].T @ x)
            old, nrm = nrm, np.linalg.norm(x)
            if nrm > 0.5 * old:
                break
        V[:, j] = x / nrm
        Mh[:j + 1, j] = V[:, :j + 1].T @ mv(V[:, j])
        Mh[j, :j + 1] = Mh[:j + 1, j]
        j += 1
        it += 1
        if time.perf_counter() - t0 > budget_s:
            timed_out = True
            break
    return {"kconv": k, "lambda": [float(x) for x in lam], "it": it, "it_inner": inner,
            "wall_s": time.perf_counter() - t0, "stopped_at_budget": timed_out}


def end_to_end(name, A, K, n, itmax, budget_s):
    from pysparse_amd.eigen import jdsym
    from pysparse_amd.itsolvers import krylov
    from pysparse_amd import _capi
    jdsym.jdsym(A, None, K, 1, 0.0, 1e-8, 2, krylov.qmrs)  # warm-up: code objects, pool vectors, lazily built tables
    _capi.lib().psp_synchronize()
    walls, res = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        res = jdsym.jdsym(A, None, K, 5, 0.0, 1e-8, itmax, krylov.qmrs)
        walls.append(time.perf_counter() - t0)
    dev_row = {"kconv": res[0], "lambda": [float(x) for x in res[1]], "it": res[3], "it_inner": res[4],
               "wall_s_median": statistics.median(walls), "wall_s_all": walls}
    host_row = host_jdsym(A, K, n, 5, 0.0, 1e-8, itmax, krylov.qmrs, budget_s=budget_s)
    row = {"case": name, "n": n, "kmax": 5, "tau": 0.0, "jdtol": 1e-8, "itmax": itmax, "linsolver": "qmrs", "K": "jacobi",
           "device": dev_row, "host_loop": host_row}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jdsym_timing.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes: checks that the tool runs, measures nothing useful")
    ap.add_argument("--budget", type=float, default=120.0, help="wall-time budget of each host-loop baseline, seconds")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401 -- its HIP runtime first (pysparse_amd/_capi.py)
    except ImportError:
        pass
    from pysparse_amd import _capi, device as dev
    from pysparse_amd.precon import precon
    from pysparse_amd.sparse import spmatrix
    from pysparse_amd.tools import standins
    L = _capi.lib()
    name, cus, _ = dev.device_info()
    out = {"device": name, "compute_units": cus, "build_id": L.psp_build_id().decode()}
    out["kernels"] = kernels(L, dev, 1 << (18 if a.quick else 24), [8, 16, 32])
    L.psp_trim()
    rows = []
    g = 64 if a.quick else 512
    P = spmatrix.poisson_csr(g, g)
    rows.append(end_to_end("poisson_csr(%d, %d)" % (g, g), P, precon.jacobi(P), g * g, 40 if a.quick else 400, a.budget))
    n, ind, col, val, diag = standins.fem_sss_arrays(*((12, 12, 12) if a.quick else ()), shuffle=32)
    S = spmatrix.sss_from_arrays(ind, col, val, diag)
    rows.append(end_to_end("standin:fem32", S, precon.jacobi(S), n, 40 if a.quick else 400, a.budget))
    out["end_to_end"] = rows
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
