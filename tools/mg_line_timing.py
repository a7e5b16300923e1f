"""Timing of precon.multigrid(..., galerkin=True, line=a) (pysparse_amd/csrc/psp_mg_line.h) -> profiles/mg_line_timing.json.

Per grid (128^3, 256^3, 512^3, 4096^2) and per operator -- the finite-volume Laplacian on a tensor mesh whose last axis is
graded (cell widths h_i ~ 10^4^(i / (n - 1)), normalised to sum 1) and the one with uniform cells -- uploaded as a csr_mat:

1. Creation of the line handle (line = the last axis) and of the point-smoothed galerkin=True handle: host clock.
2. One V-cycle of each (psp_mg_precon_dev, omega 0.8, steps 2) with tools/mg_timing.py's protocol (device-event time, median
   of 5 windows), the two handles alternating twice in one process; the bytes of DESIGN.md section 9h's model; that rate over
   psp_stream_probe (2 read streams + 1 write stream) in the same process.
3. Time to solution: psp_pcg_dev to 1e-8 on a seeded random right-hand side with precon.jacobi, the point handle and the
   line handle, alternating twice, iteration counts and the true relative residual of each.  The yardstick is the point
   handle: the library's best for these matrices before.
4. --axes (256^3 by default): the cycle time with line = 0 and line = 1 on the uniform operator (line 0 is the strided form
   of the kernels).

Every case runs in a child process of its own under `timeout`; the first child that fails ends the run.
--trace GRID runs one cycle of the line handle on the graded operator and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --`.

    python tools/mg_line_timing.py [--out profiles/mg_line_timing.json] [--quick] [--grids 128^3,256^3] [--trace 256^3]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mg_timing import cycle_time  # noqa: E402
from mg_galerkin_timing import fill_random  # noqa: E402
from mg_galerkin_timing import model_bytes as model_bytes_point  # noqa: E402

CASES = {"128^3": ((128, 128, 128), 400), "256^3": ((256, 256, 256), 700), "4096^2": ((4096, 4096), 700),
         "512^3": ((512, 512, 512), 1150)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}
RATIO = 1.0e4


def widths(n, ratio):
    if ratio == 1.0:
        return np.full(n, 1.0 / n)
    h = ratio ** (np.arange(n, dtype=np.float64) / (n - 1))
    return h / h.sum()


def mesh_operator(grid, ratio):
    """CSR arrays (int32 ind, int32 col, float64 val) of A = sum_a (x)_b (T1_a if b = a else diag(h_b)) on the tensor mesh
    whose last axis has graded cells (ratio) and whose other axes have uniform ones; T1_a = tridiag(-t_i, t_i + t_{i+1},
    -t_{i+1}) with the face weights t_0 = 2 / h_0, t_i = 2 / (h_{i-1} + h_i), t_n = 2 / h_{n-1}.  Rows sorted by column, a
    pair of couplings is one number stored twice."""
    nd, n = len(grid), int(np.prod(grid))
    shape = tuple(grid)[::-1]  # axis 0 of the grid is the fastest index
    hs = [widths(m, ratio if a == nd - 1 else 1.0) for a, m in enumerate(grid)]
    stride = [int(np.prod(grid[:a])) for a in range(nd)]

    def along(a, v):
        sh = [1] * nd
        sh[nd - 1 - a] = v.size
        return v.reshape(sh)

    val = np.zeros(shape + (2 * nd + 1,))
    have = np.zeros(shape + (2 * nd + 1,), dtype=bool)
    off = np.zeros(2 * nd + 1, dtype=np.int64)
    for a in range(nd):
        h, m = hs[a], grid[a]
        t = np.empty(m + 1)
        t[0], t[m] = 2.0 / h[0], 2.0 / h[m - 1]
        t[1:m] = 2.0 / (h[:-1] + h[1:])
        vol = np.ones([1] * nd)
        for b in range(nd):
            if b != a:
                vol = vol * along(b, hs[b])
        ax = nd - 1 - a
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[ax], hi[ax] = slice(0, m - 1), slice(1, m)
        lo, hi = tuple(lo), tuple(hi)
        val[..., nd] += along(a, t[:-1] + t[1:]) * vol
        c = np.broadcast_to(-(along(a, t[1:m]) * vol), val[hi + (0,)].shape)
        sl, su = nd - 1 - a, nd + 1 + a
        off[sl], off[su] = -stride[a], stride[a]
        val[hi + (sl,)] = c
        have[hi + (sl,)] = True
        val[lo + (su,)] = c
        have[lo + (su,)] = True
    have[..., nd] = True
    have = have.reshape(n, 2 * nd + 1)
    ind = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(have.sum(axis=1), out=ind[1:])
    assert ind[-1] < 2 ** 31 - 8192
    col = (np.arange(n, dtype=np.int64)[:, None] + off[None, :])[have].astype(np.int32)
    return ind.astype(np.int32), col, val.reshape(n, 2 * nd + 1)[have]


def model_bytes(dims, steps, nd):
    """bytes one application of a line handle moves through memory by the kernels' own reads and writes (the
    neighbours' rows of x and of the lower arrays come from the caches).  A level stores C = 1 + lower arrays coefficient
    arrays (ND + 1 on level 0, (3^ND + 1) / 2 below), of which l is one, and q.  The first sweep of a level: forward reads
    b, l, q and writes y, backward reads y, q, l and writes x (8 per point).  A further sweep: forward reads x, b, the C
    arrays and q and writes y, backward reads y, q, l, x and writes x (C + 9).  The restriction reads x, b and the C arrays
    and writes b_c; the prolongation reads x and e and writes x.  The last level is one first sweep."""
    total = 0.0
    nl = len(dims)
    for l in range(nl - 1):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        c = (nd + 1) if l == 0 else (3 ** nd + 1) // 2
        total += 8.0 * (8 * n + (2 * steps - 1) * (c + 9) * n + ((2 + c) * n + nc) + (2 * n + nc))
    return total + 8.0 * 8 * float(np.prod(dims[nl - 1]))


def true_relres(L, check, A, xb, bb, rb, n):
    A.matvec_dev(xb.ptr, rb.ptr)
    res2 = b2 = 0.0
    chunk = 1 << 24
    for k in range(0, n, chunk):
        m = min(chunk, n - k)
        r, b = np.empty(m), np.empty(m)
        check(L.psp_memcpy_d2h(r.ctypes.data, rb.ptr + 8 * k, 8 * m))
        check(L.psp_memcpy_d2h(b.ctypes.data, bb.ptr + 8 * k, 8 * m))
        res2 += float(((b - r) ** 2).sum())
        b2 += float((b ** 2).sum())
    return (res2 / b2) ** 0.5


def upload(grid, ratio):
    from pysparse_amd import device as dev
    n = int(np.prod(grid))
    ind, col, val = mesh_operator(grid, ratio)
    return dev.DeviceCSR.from_arrays((n, n), ind, col, val)


def run_operator(name, grid, ratio, axes):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    nd, n = len(grid), int(np.prod(grid))
    A = upload(grid, ratio)
    check(L.psp_synchronize())
    t = time.perf_counter()
    Kl = dev.DeviceMultigridLine(A, grid, 0.8, 2, line=nd - 1)
    check(L.psp_synchronize())
    t_line = time.perf_counter() - t
    t = time.perf_counter()
    Kp = dev.DeviceMultigrid(A, grid, 0.8, 2, galerkin=True)
    check(L.psp_synchronize())
    t_point = time.perf_counter() - t
    J = dev.DeviceJacobi(A)
    il, ip = Kl.info(), Kp.info()
    out = {"ratio": ratio, "line": {"levels": il["levels"], "launches_per_apply": il["launches_per_apply"],
                                    "creation_seconds": t_line, "bytes": Kl.bytes(),
                                    "operator_bytes_per_fine_point": Kl.bytes()["operator"] / n,
                                    "vector_bytes_per_fine_point": Kl.bytes()["vector"] / n},
           "point": {"levels": ip["levels"], "tail_first_level": ip["tail_first_level"],
                     "launches_per_apply": ip["launches_per_apply"], "creation_seconds": t_point, "bytes": Kp.bytes()}}
    bb, xb, rb = dev.DeviceBuffer(n), dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    fill_random(L, check, bb, n)
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    cyc = {"line": [], "point": []}
    for rnd in range(2):
        for label, K in (("line", Kl), ("point", Kp)):
            cyc[label].append(cycle_time(L, K, bb, xb, min_total_s=0.3))
    mbl = model_bytes(il["dims"], 2, nd)
    mbp = model_bytes_point(ip["dims"], ip["tail_first_level"], 2, nd)
    best = {k: min(c["median_ms"] for c in v) for k, v in cyc.items()}
    out["vcycle"] = {"line": cyc["line"], "point": cyc["point"], "line_model_bytes": mbl, "point_model_bytes": mbp,
                     "line_model_bytes_per_fine_point": mbl / n, "line_GBps_model": mbl / best["line"] / 1e6,
                     "line_fraction_of_stream_probe": mbl / best["line"] / 1e6 / probe,
                     "point_GBps_model": mbp / best["point"] / 1e6,
                     "time_ratio_line_over_point": best["line"] / best["point"]}
    print(json.dumps({"grid": name, "ratio": ratio, "vcycle_ms": best}), flush=True)
    aop = dev._Op(A, "matvec")
    ops = (("jacobi", dev._Op(J, "precon")), ("point", dev._Op(Kp, "precon")), ("line", dev._Op(Kl, "precon")))
    solves = {k: [] for k, _ in ops}
    for rnd in range(2):
        for label, op in ops:
            xb.zero()
            i, it, rr = C.c_int(), C.c_int(), C.c_double()
            check(L.psp_synchronize())
            t = time.perf_counter()
            check(L.psp_pcg_dev(aop._h, op._h, n, xb.ptr, bb.ptr, 1e-8, 100000, C.byref(i), C.byref(it), C.byref(rr), None))
            check(L.psp_synchronize())
            dt = time.perf_counter() - t
            solves[label].append({"seconds": dt, "info": i.value, "iter": it.value, "relres": rr.value,
                                  "true_relres": true_relres(L, check, A, xb, bb, rb, n)})
            print(json.dumps({"grid": name, "ratio": ratio, "pcg": label, **solves[label][-1]}), flush=True)
    tp, tl = [s["seconds"] for s in solves["point"]], [s["seconds"] for s in solves["line"]]
    out["pcg_to_1e-8"] = dict(solves, time_ratio_point_over_line=min(tp) / min(tl),
                              time_ratio_spread=[min(tp) / max(tl), max(tp) / min(tl)])
    if axes:
        del Kp, J, ops
        out["line_axes"] = {str(nd - 1): best["line"]}
        for a in range(nd - 1):
            Ka = dev.DeviceMultigridLine(A, grid, 0.8, 2, line=a)
            out["line_axes"][str(a)] = cycle_time(L, Ka, bb, xb, min_total_s=0.3)["median_ms"]
            Ka.close()
    return out


def run_case(name, grid, axes):
    from pysparse_amd import device as dev
    out = {"grid": list(grid), "n": int(np.prod(grid)), "device": dev.device_info()[0], "line_axis": len(grid) - 1}
    out["graded"] = run_operator(name, grid, RATIO, False)
    out["uniform"] = run_operator(name, grid, 1.0, axes)
    return out


def trace(grid):
    """one warm-up cycle and one traced-by-whoever-runs-this cycle of the line handle on the graded operator"""
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    n = int(np.prod(grid))
    A = upload(grid, RATIO)
    K = dev.DeviceMultigridLine(A, grid, 0.8, 2, line=len(grid) - 1)
    bb, xb = dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    fill_random(lib(), check, bb, n)
    for _ in range(3):
        K.precon_dev(bb.ptr, xb.ptr)
    check(lib().psp_synchronize())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_line_timing.json"))
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--grids", help="comma-separated subset of the grids; results are merged into --out")
    p.add_argument("--axes", default="256^3", help="the grid that also times line = 0 .. ND - 2")
    p.add_argument("--trace", help="run three cycles of the line handle on this grid and exit")
    p.add_argument("--case", help="(internal) run one grid in this process and print its JSON record")
    a = p.parse_args()
    cases = QUICK if a.quick else CASES
    if a.trace:
        trace(cases[a.trace][0])
        return 0
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, cases[a.case][0], a.case == a.axes or a.quick)), flush=True)
        return 0
    res = {"quick": a.quick, "cases": {}}
    if a.grids and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    for name, (grid, limit) in cases.items():
        if a.grids and name not in a.grids.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name, "--axes", a.axes]
        if a.quick:
            cmd.append("--quick")
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("mg_line_timing: %s ended with status %d; nothing further is started" % (name, r.returncode), flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        res["cases"][name] = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
