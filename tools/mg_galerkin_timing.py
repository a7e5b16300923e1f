"""Timing of precon.multigrid(..., galerkin=True) (pysparse_amd/csrc/psp_mg_galerkin.h) -> profiles/mg_galerkin_timing.json.

Per grid (128^3, 256^3, 512^3, 4096^2), on a seeded smooth-kappa operator -div(kappa grad u) built here (kappa =
exp(sum_a (3 / ND) sin(2 pi x_a + phi_a)), max / min about 400; couplings = harmonic means; Dirichlet ends) and uploaded as
a csr_mat:

1. Creation of the handle (the checking pass, the Galerkin products, the coarsest inverse): host clock, once.
2. One V-cycle (psp_mg_precon_dev, omega 0.8, steps 2) with tools/mg_timing.py's protocol: device-event time per application
   after a warm-up, median of windows that together hold at least 0.5 s; the bytes of DESIGN.md section 9d's model
   (model_bytes below); that rate over psp_stream_probe (2 read streams + 1 write stream) in the same process.
3. Time to solution: psp_pcg_dev to 1e-8 on a seeded random right-hand side, precon.jacobi and the Galerkin cycle
   alternating twice in one process, iteration counts and the true relative residual of each.  Jacobi-PCG is what the
   library had for these matrices before: it is the yardstick.
4. On the constant-coefficient operator of the same grid: the Galerkin cycle beside the matrix-free cycle of section 9c.

Every grid runs in a child process of its own under `timeout`; the first child that fails ends the run.

--precision single measures the float32 cycle of DESIGN.md section 9g (device.DeviceMultigrid32) with that section's byte
model; the default output file then is profiles/mg_galerkin_timing_single.json.

    python tools/mg_galerkin_timing.py [--out profiles/mg_galerkin_timing.json] [--quick] [--grids 128^3,256^3]
                                       [--precision double|single]
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
from mg_timing import model_bytes as model_bytes_matrix_free  # noqa: E402

CASES = {"128^3": ((128, 128, 128), 300), "256^3": ((256, 256, 256), 500), "4096^2": ((4096, 4096), 600),
         "512^3": ((512, 512, 512), 1100)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}


def smooth_operator(grid, seed=0):
    """CSR arrays (int32 ind, int32 col, float64 val) of the smooth-kappa operator, rows sorted by column; kappa is a product
    of one factor per axis, so that the field costs one pass"""
    nd, n = len(grid), int(np.prod(grid))
    rng = np.random.default_rng([seed, nd] + list(grid))
    shape = tuple(grid)[::-1]  # axis 0 of the grid is the fastest index
    kap = np.ones(shape)
    for ax, m in enumerate(shape):
        x = (np.arange(m) + 0.5) / m
        sh = [1] * nd
        sh[ax] = m
        kap = kap * np.exp(3.0 / nd * np.sin(2.0 * np.pi * x + rng.uniform(0.0, 2.0 * np.pi))).reshape(sh)
    stride = [int(np.prod(grid[:a])) for a in range(nd)]
    # slots in column order: -st_{nd-1}, ..., -st_0, 0, +st_0, ..., +st_{nd-1}
    val = np.zeros(shape + (2 * nd + 1,))
    have = np.zeros(shape + (2 * nd + 1,), dtype=bool)
    off = np.zeros(2 * nd + 1, dtype=np.int64)
    diag = np.zeros(shape)
    for a in range(nd):
        ax = nd - 1 - a
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[ax], hi[ax] = slice(0, grid[a] - 1), slice(1, grid[a])
        lo, hi = tuple(lo), tuple(hi)
        h = 2.0 * kap[lo] * kap[hi] / (kap[lo] + kap[hi])
        low, up = kap.copy(), kap.copy()
        low[hi] = h
        up[lo] = h
        diag += low + up
        sl, su = nd - 1 - a, nd + 1 + a
        off[sl], off[su] = -stride[a], stride[a]
        val[hi + (sl,)] = -h
        have[hi + (sl,)] = True
        val[lo + (su,)] = -h
        have[lo + (su,)] = True
    val[..., nd] = diag
    have[..., nd] = True
    have = have.reshape(n, 2 * nd + 1)
    ind = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(have.sum(axis=1), out=ind[1:])
    assert ind[-1] < 2 ** 31 - 8192
    col = (np.arange(n, dtype=np.int64)[:, None] + off[None, :])[have].astype(np.int32)
    return ind.astype(np.int32), col, val.reshape(n, 2 * nd + 1)[have]


def model_bytes(dims, tail_first, steps, nd, single=False):
    """bytes one application moves through memory by the kernels' own reads and writes (the neighbours' rows
    of x and of the lower arrays come from the caches).  A level stores C = 1 + lower arrays coefficient arrays (ND + 1 on
    level 0, (3^ND + 1) / 2 below) and w.  Per level above the tail: the first pass (reads b, w and the C arrays, writes x),
    every further sweep (reads x, b, w, C arrays, writes x), the restriction (reads x, b, C arrays, writes b_c), the
    prolongation (reads x and e, writes x); the tail reads its b and writes its x (its coefficient arrays are a few hundred
    kilobytes that stay in the L2 cache).  single: every array and level vector is 4 B per point; the finest
    level's b stays the caller's 8 B wherever it is read, and its last sweep writes the caller's 8 B."""
    e = 4 if single else 8
    total = 0.0
    for l in range(tail_first):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        c = (nd + 1) if l == 0 else (3 ** nd + 1) // 2
        eb = 8 if l == 0 else e
        first = (eb + e * (2 + c)) * n if steps >= 2 else (eb + 2 * e) * n
        sweeps = max(steps - 2, 0) + steps
        total += first + sweeps * (eb + e * (3 + c)) * n + ((eb + e * (1 + c)) * n + e * nc) + (2 * e * n + e * nc)
        if l == 0:
            total += (8 - e) * n
    return total + (16.0 if tail_first == 0 else 2.0 * e) * float(np.prod(dims[tail_first]))


def fill_random(L, check, buf, n, seed=0):
    g = np.random.default_rng(seed)
    chunk = 1 << 24
    for k in range(0, n, chunk):
        v = g.standard_normal(min(chunk, n - k))
        check(L.psp_memcpy_h2d(buf.ptr + 8 * k, v.ctypes.data, 8 * v.size))


def run_case(name, grid, precision="double"):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    nd, n = len(grid), int(np.prod(grid))
    single = precision == "single"
    Multigrid = dev.DeviceMultigrid32 if single else dev.DeviceMultigrid
    t = time.perf_counter()
    ind, col, val = smooth_operator(grid)
    t_host = time.perf_counter() - t
    A = dev.DeviceCSR.from_arrays((n, n), ind, col, val)
    del ind, col, val
    check(L.psp_synchronize())
    t = time.perf_counter()
    K = Multigrid(A, grid, 0.8, 2, galerkin=True)
    check(L.psp_synchronize())
    t_create = time.perf_counter() - t
    J = dev.DeviceJacobi(A)
    info = K.info()
    out = {"grid": list(grid), "n": n, "device": dev.device_info()[0], "levels": info["levels"],
           "tail_first_level": info["tail_first_level"], "launches_per_apply": info["launches_per_apply"],
           "operator": "smooth kappa, seed 0", "host_assembly_seconds": t_host, "handle_creation_seconds": t_create,
           "precision": info["precision"], "bytes": K.bytes()}
    bb, xb = dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    fill_random(L, check, bb, n)
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    cyc = cycle_time(L, K, bb, xb)
    mb = model_bytes(info["dims"], info["tail_first_level"], 2, nd, single)
    cyc.update({"model_bytes": mb, "model_bytes_per_fine_point": mb / n, "GBps_model": mb / cyc["median_ms"] / 1e6,
                "fraction_of_stream_probe": mb / cyc["median_ms"] / 1e6 / probe})
    out["vcycle"] = cyc
    print(json.dumps({"grid": name, "vcycle": cyc}), flush=True)
    # time to solution, alternating
    aop, jop, kop = dev._Op(A, "matvec"), dev._Op(J, "precon"), dev._Op(K, "precon")
    rb = dev.DeviceBuffer(n)
    chunk = 1 << 24
    solves = {"jacobi": [], "galerkin_multigrid": []}
    for rnd in range(2):
        for label, op in (("jacobi", jop), ("galerkin_multigrid", kop)):
            xb.zero()
            i, it, rr = C.c_int(), C.c_int(), C.c_double()
            check(L.psp_synchronize())
            t = time.perf_counter()
            check(L.psp_pcg_dev(aop._h, op._h, n, xb.ptr, bb.ptr, 1e-8, 100000, C.byref(i), C.byref(it), C.byref(rr), None))
            check(L.psp_synchronize())
            dt = time.perf_counter() - t
            A.matvec_dev(xb.ptr, rb.ptr)
            res2 = b2 = 0.0
            for k in range(0, n, chunk):
                m = min(chunk, n - k)
                r, b = np.empty(m), np.empty(m)
                check(L.psp_memcpy_d2h(r.ctypes.data, rb.ptr + 8 * k, 8 * m))
                check(L.psp_memcpy_d2h(b.ctypes.data, bb.ptr + 8 * k, 8 * m))
                res2 += float(((b - r) ** 2).sum())
                b2 += float((b ** 2).sum())
            solves[label].append({"seconds": dt, "info": i.value, "iter": it.value, "relres": rr.value,
                                  "true_relres": (res2 / b2) ** 0.5})
            print(json.dumps({"grid": name, "pcg": label, **solves[label][-1]}), flush=True)
    tj = [s["seconds"] for s in solves["jacobi"]]
    tm = [s["seconds"] for s in solves["galerkin_multigrid"]]
    out["pcg_to_1e-8"] = {"jacobi": solves["jacobi"], "galerkin_multigrid": solves["galerkin_multigrid"],
                          "time_ratio_jacobi_over_multigrid": min(tj) / min(tm),
                          "time_ratio_spread": [min(tj) / max(tm), max(tj) / min(tm)],
                          "iteration_ratio_jacobi_over_multigrid":
                              solves["jacobi"][0]["iter"] / solves["galerkin_multigrid"][0]["iter"]}
    del K, J, A, aop, jop, kop
    # the constant-coefficient operator: the Galerkin cycle beside the matrix-free one
    Ac = dev.DeviceCSR.poisson(*grid)
    Kg = Multigrid(Ac, grid, 0.8, 2, galerkin=True)
    Km = Multigrid(Ac, grid, 0.8, 2)
    cg, cm = cycle_time(L, Kg, bb, xb), cycle_time(L, Km, bb, xb)
    mm = model_bytes_matrix_free(info["dims"], info["tail_first_level"], 2, single)
    out["constant_coefficients"] = {"galerkin_cycle": cg, "matrix_free_cycle": cm, "matrix_free_model_bytes": mm,
                                    "galerkin_model_bytes": mb, "time_ratio_galerkin_over_matrix_free":
                                        cg["median_ms"] / cm["median_ms"], "byte_ratio": mb / mm}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out")
    p.add_argument("--precision", choices=["double", "single"], default="double")
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--grids", help="comma-separated subset of the grids; results are merged into --out")
    p.add_argument("--case", help="(internal) run one grid in this process and print its JSON record")
    a = p.parse_args()
    if not a.out:
        a.out = os.path.join(ROOT, "profiles",
                             "mg_galerkin_timing.json" if a.precision == "double" else "mg_galerkin_timing_single.json")
    cases = QUICK if a.quick else CASES
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, cases[a.case][0], a.precision)), flush=True)
        return 0
    res = {"quick": a.quick, "precision": a.precision, "cases": {}}
    if a.grids and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    for name, (grid, limit) in cases.items():
        if a.grids and name not in a.grids.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name,
               "--precision", a.precision]
        if a.quick:
            cmd.append("--quick")
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("mg_galerkin_timing: %s ended with status %d; nothing further is started" % (name, r.returncode), flush=True)
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
