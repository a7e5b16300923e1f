"""Timing of precon.multigrid(..., galerkin=True, interp='operator') -> profiles/mg_interp_timing.json.

Per grid (256^3, 4096^2, 128^3) and per coefficient field, on -div(kappa grad u) with harmonic face averages and Dirichlet
ends (5 / 7 points, built here and uploaded as a csr_mat), with the protocol of tools/mg_galerkin_timing.py:

  block   kappa = 1 but for random blocks of 8 cells a side that hold 1e4 (each with probability 0.3): what the feature is for
  smooth  kappa = exp(sum of sines), ratio about 400: what the feature costs where it is not needed

1. Creation of the handle with interp='operator' and of the one with interp='linear' (the parent's handle): host clock,
   once each, after a throwaway handle of each kind has taken the library's first-use costs; what each holds at rest
   (psp_mg_bytes).
2. One V-cycle (psp_mg_precon_dev, omega 0.8, steps 2) of both, alternating twice in the same process: device-event time,
   median of 5 windows; the byte models; psp_stream_probe (2 read streams + 1 write stream) in the same process.
3. Time to solution: psp_pcg_dev to 1e-8 on a seeded random right-hand side with precon.jacobi, the linear handle and the
   operator handle, alternating twice in one process; iteration counts and the true relative residual of each.

Every case runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python tools/mg_interp_timing.py [--out profiles/mg_interp_timing.json] [--quick] [--grids 256^3,4096^2] [--fields block,smooth] [--creation-only]
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
from mg_galerkin_timing import model_bytes as model_bytes_linear  # noqa: E402

CASES = {"256^3": ((256, 256, 256), 1100), "4096^2": ((4096, 4096), 900), "128^3": ((128, 128, 128), 600)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}
FIELDS = ("block", "smooth")
JACOBI_MAXIT = 20000


def kappa(grid, field, seed=0):
    """the cell field, shape grid[::-1]"""
    shape = tuple(grid)[::-1]
    rng = np.random.default_rng([seed, len(grid)] + list(grid))
    if field == "block":
        k = rng.random(tuple(-(-m // 8) for m in shape)) < 0.3
        for ax in range(len(shape)):
            k = np.repeat(k, 8, axis=ax)
        return np.where(k[tuple(slice(0, m) for m in shape)], 1.0e4, 1.0)
    t = np.zeros(shape)
    for ax, m in enumerate(shape):
        x = (np.arange(m) + 0.5) / m
        sh = [1] * len(shape)
        sh[ax] = m
        t = t + np.sin(2.0 * np.pi * x + rng.uniform(0.0, 2.0 * np.pi)).reshape(sh)
    return np.exp(3.0 / len(shape) * t)


def operator(grid, kap):
    """CSR arrays (int32 ind, int32 col, float64 val): the coupling of two neighbours is minus the harmonic mean of their
    kappa, a missing neighbour counts with the cell's own kappa on the diagonal; rows sorted by column"""
    nd, n = len(grid), int(np.prod(grid))
    flat = kap.reshape(-1)
    st = np.cumprod((1,) + tuple(grid[:-1])).astype(np.int64)
    r = np.arange(n, dtype=np.int64)
    co = [(r // st[a]) % grid[a] for a in range(nd)]
    diag = np.zeros(n)
    lower, upper = [], []
    for a in range(nd):
        has_lo, has_up = co[a] > 0, co[a] < grid[a] - 1
        nb = flat[np.where(has_up, r + st[a], r)]
        h_up = np.where(has_up, 2.0 * flat * nb / (flat + nb), 0.0)   # the coupling to the upper neighbour
        h_lo = np.zeros(n)
        h_lo[st[a]:] = h_up[:n - st[a]]
        h_lo[~has_lo] = 0.0
        diag += np.where(has_lo, h_lo, flat) + np.where(has_up, h_up, flat)
        lower.append((has_lo, -st[a], -h_lo))
        upper.append((has_up, st[a], -h_up))
    parts = lower[::-1] + [(np.ones(n, dtype=bool), 0, diag)] + upper  # ascending column
    have = np.stack([p[0] for p in parts], axis=1)
    ind = np.concatenate([[0], np.cumsum(have.sum(axis=1))])
    assert ind[-1] < 2 ** 31 - 8192
    col = (r[:, None] + np.array([p[1] for p in parts], dtype=np.int64)[None, :])[have].astype(np.int32)
    val = np.stack([p[2] for p in parts], axis=1)[have]
    return ind.astype(np.int32), col, val


def model_bytes_operator(dims, steps, nd):
    """tools/mg_galerkin_timing.model_bytes with every level above the last through launches and the weighted transfers:
    the restriction also reads the 2^ND weight arrays of the level, and so does the prolongation; the dense product of the
    last level reads its b and writes its x"""
    total = 0.0
    for l in range(len(dims) - 1):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        c = (nd + 1) if l == 0 else (3 ** nd + 1) // 2
        wts = 2 ** nd
        first = 8 * (3 + c) * n if steps >= 2 else 24 * n
        sweeps = max(steps - 2, 0) + steps
        total += first + sweeps * 8 * (4 + c) * n + (8 * (2 + c + wts) * n + 8 * nc) + (8 * (2 + wts) * n + 8 * nc)
    return total + 16.0 * float(np.prod(dims[-1]))


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


def run_case(name, grid, field, creation_only=False):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    nd, n = len(grid), int(np.prod(grid))
    t = time.perf_counter()
    ind, col, val = operator(grid, kappa(grid, field))
    t_host = time.perf_counter() - t
    nnz = int(ind[-1])
    A = dev.DeviceCSR.from_arrays((n, n), ind, col, val)
    del ind, col, val
    out = {"grid": list(grid), "n": n, "nnz": nnz, "field": field, "device": dev.device_info()[0], "host_assembly_seconds": t_host}
    handles = {}
    # a throwaway handle of each kind first: it takes the first-use costs of the library (module load, the first large
    # allocations), so that the two timed creations below are comparable
    for interp in ("linear", "operator"):
        dev.DeviceMultigridInterp(A, grid, 0.8, 2, interp=interp).close()
    for label, interp in (("linear", "linear"), ("operator", "operator")):
        check(L.psp_synchronize())
        t = time.perf_counter()
        K = dev.DeviceMultigridInterp(A, grid, 0.8, 2, interp=interp)
        check(L.psp_synchronize())
        info = K.info()
        handles[label] = K
        out[label] = {"handle_creation_seconds": time.perf_counter() - t, "bytes": K.bytes(), "levels": info["levels"],
                      "tail_first_level": info["tail_first_level"], "launches_per_apply": info["launches_per_apply"]}
        out[label]["bytes"]["operator_per_fine_point"] = out[label]["bytes"]["operator"] / n
    out["operator"]["fallbacks"] = [handles["operator"].interp_fallbacks(l) for l in range(out["operator"]["levels"] - 1)]
    if creation_only:
        return out
    bb, xb = dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    fill_random(L, check, bb, n)
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    rounds = {"linear": [], "operator": []}
    for rnd in range(2):
        for label in ("operator", "linear"):
            rounds[label].append(cycle_time(L, handles[label], bb, xb))
            print(json.dumps({"grid": name, "field": field, "cycle": label, **rounds[label][-1]}), flush=True)
    dims = handles["linear"].info()["dims"]
    ml = model_bytes_linear(dims, out["linear"]["tail_first_level"], 2, nd)
    mo = model_bytes_operator(dims, 2, nd)
    tl = min(r["median_ms"] for r in rounds["linear"])
    to = min(r["median_ms"] for r in rounds["operator"])
    out["vcycle"] = {"linear": rounds["linear"], "operator": rounds["operator"], "linear_model_bytes": ml,
                     "operator_model_bytes": mo, "linear_GBps_model": ml / tl / 1e6, "operator_GBps_model": mo / to / 1e6,
                     "operator_fraction_of_stream_probe": mo / to / 1e6 / probe, "time_ratio_operator_over_linear": to / tl,
                     "byte_ratio_operator_over_linear": mo / ml}
    J = dev.DeviceJacobi(A)
    aop = dev._Op(A, "matvec")
    ops = {"jacobi": dev._Op(J, "precon"), "linear": dev._Op(handles["linear"], "precon"),
           "operator": dev._Op(handles["operator"], "precon")}
    rb = dev.DeviceBuffer(n)
    solves = {k: [] for k in ops}
    for rnd in range(2):
        for label, op in ops.items():
            if label == "jacobi" and rnd == 1 and solves["jacobi"][0]["info"] != 0:
                continue  # it did not converge within JACOBI_MAXIT: once is enough
            xb.zero()
            i, it, rr = C.c_int(), C.c_int(), C.c_double()
            check(L.psp_synchronize())
            t = time.perf_counter()
            check(L.psp_pcg_dev(aop._h, op._h, n, xb.ptr, bb.ptr, 1e-8, JACOBI_MAXIT if label == "jacobi" else 5000,
                                C.byref(i), C.byref(it), C.byref(rr), None))
            check(L.psp_synchronize())
            dt = time.perf_counter() - t
            solves[label].append({"seconds": dt, "info": i.value, "iter": it.value, "relres": rr.value,
                                  "true_relres": true_relres(L, check, A, xb, bb, rb, n)})
            print(json.dumps({"grid": name, "field": field, "pcg": label, **solves[label][-1]}), flush=True)
    best = {k: min(s["seconds"] for s in v) for k, v in solves.items()}
    out["pcg_to_1e-8"] = dict(solves, time_ratio_linear_over_operator=best["linear"] / best["operator"],
                              time_ratio_jacobi_over_operator=best["jacobi"] / best["operator"])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_interp_timing.json"))
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--grids", help="comma-separated subset of the grids; results are merged into --out")
    p.add_argument("--fields", default=",".join(FIELDS), help="comma-separated subset of block, smooth")
    p.add_argument("--creation-only", action="store_true",
                   help="stop after the handles exist: handle_creation_seconds and bytes, no cycles and no solves")
    p.add_argument("--case", help="(internal) run one grid:field in this process and print its JSON record")
    a = p.parse_args()
    cases = QUICK if a.quick else CASES
    if a.case:
        name, field = a.case.split(":")
        print("RESULT " + json.dumps(run_case(name, cases[name][0], field, a.creation_only)), flush=True)
        return 0
    res = {"quick": a.quick, "cases": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    for name, (grid, limit) in cases.items():
        if a.grids and name not in a.grids.split(","):
            continue
        for field in a.fields.split(","):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name + ":" + field]
            if a.quick:
                cmd.append("--quick")
            if a.creation_only:
                cmd.append("--creation-only")
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                print("mg_interp_timing: %s %s ended with status %d; nothing further is started" % (name, field, r.returncode),
                      flush=True)
                return 1
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            res["cases"][name + ":" + field] = json.loads(line[len("RESULT "):])
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
