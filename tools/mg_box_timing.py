"""Timing of precon.multigrid(..., galerkin=True, stencil='box') -> profiles/mg_box_timing.json.

Per grid (256^3, 4096^2), on the constant-coefficient Q1 (bilinear / trilinear) Laplacian with Dirichlet ends, built here
with all 3^ND entries of a row stored (the face couplings of the trilinear form are 0 and stored as such) and uploaded as
a csr_mat, with the protocol of tools/mg_galerkin_timing.py:

1. Creation of the box handle (the checking pass, the Galerkin products, the coarsest inverse): host clock, once; what it
   holds at rest (psp_mg_bytes).
2. One V-cycle (psp_mg_precon_dev, omega 0.8, steps 2) of the box handle and, alternating with it twice in the same process,
   of an axis handle (galerkin=True) on the 5- / 7-point Poisson operator of the same grid: the yardstick for what the
   9- / 27-point level 0 costs.  Device-event time, median of 5 windows; the byte model of section 9i; that rate over
   psp_stream_probe (2 read streams + 1 write stream) in the same process.
3. Time to solution: psp_pcg_dev to 1e-8 on a seeded random right-hand side, precon.jacobi and the box handle alternating
   twice in one process, iteration counts and the true relative residual of each.

512^3 is not run: its 27-point CSR form has 3.6e9 entries, more than the library's 32-bit row pointers hold.  Every grid
runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python tools/mg_box_timing.py [--out profiles/mg_box_timing.json] [--quick] [--grids 256^3,4096^2]
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
from mg_galerkin_timing import model_bytes as model_bytes_axis  # noqa: E402

CASES = {"256^3": ((256, 256, 256), 1100), "4096^2": ((4096, 4096), 900)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}


def q1_operator(grid, rows_per_chunk=1 << 21):
    """CSR arrays (int32 ind, int32 col, float64 val) of sum_a (x)_b (K1 if b == a else M1), K1 = [-1 2 -1],
    M1 = [1 4 1] / 6, every neighbour inside the grid stored, rows sorted by column (every axis has at least 3 points)"""
    nd, n = len(grid), int(np.prod(grid))
    assert min(grid) >= 3
    g3 = tuple(grid) + (1,) * (3 - nd)
    k1, m1 = np.array([-1.0, 2.0, -1.0]), np.array([1.0, 4.0, 1.0]) / 6.0
    offs, wts, ds = [], [], []
    for d2 in ((-1, 0, 1) if nd > 2 else (0,)):
        for d1 in ((-1, 0, 1) if nd > 1 else (0,)):
            for d0 in (-1, 0, 1):
                d = (d0, d1, d2)
                w = 0.0
                for a in range(nd):
                    t = 1.0
                    for b in range(nd):
                        t = t * (k1 if b == a else m1)[d[b] + 1]
                    w += t
                offs.append(d0 + g3[0] * (d1 + g3[1] * d2))
                wts.append(w)
                ds.append(d)
    offs, wts, ds = np.array(offs, dtype=np.int64), np.array(wts), np.array(ds)
    assert np.array_equal(wts, wts[::-1])  # the weight of an offset is the weight of its mirror, bit for bit
    ind = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for k0 in range(0, n, rows_per_chunk):
        r = np.arange(k0, min(n, k0 + rows_per_chunk), dtype=np.int64)
        co = (r % g3[0], (r // g3[0]) % g3[1], r // (g3[0] * g3[1]))
        have = np.ones((r.size, offs.size), dtype=bool)
        for a in range(3):
            c = co[a][:, None] + ds[None, :, a]
            have &= (c >= 0) & (c < g3[a])
        ind[k0 + 1:k0 + 1 + r.size] = have.sum(axis=1)
        cols.append((r[:, None] + offs[None, :])[have].astype(np.int32))
        vals.append(np.broadcast_to(wts, have.shape)[have])
    np.cumsum(ind, out=ind)
    assert ind[-1] < 2 ** 31 - 8192
    return ind.astype(np.int32), np.concatenate(cols), np.concatenate(vals)


def model_bytes(dims, tail_first, steps, nd):
    """section 9d's model with level 0 stored like every lower level: C = (3^ND + 1) / 2 coefficient arrays on every level
    (14 in 3-D, 5 in 2-D) where an axis handle reads ND + 1 on level 0"""
    total = 0.0
    c = (3 ** nd + 1) // 2
    for l in range(tail_first):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        first = 8 * (3 + c) * n if steps >= 2 else 24 * n
        sweeps = max(steps - 2, 0) + steps
        total += first + sweeps * 8 * (4 + c) * n + (8 * (2 + c) * n + 8 * nc) + (16 * n + 8 * nc)
    return total + 16.0 * float(np.prod(dims[tail_first]))  # the tail reads its b and writes its x


def run_case(name, grid):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    nd, n = len(grid), int(np.prod(grid))
    t = time.perf_counter()
    ind, col, val = q1_operator(grid)
    t_host = time.perf_counter() - t
    nnz = int(ind[-1])
    A = dev.DeviceCSR.from_arrays((n, n), ind, col, val)
    del ind, col, val
    check(L.psp_synchronize())
    t = time.perf_counter()
    K = dev.DeviceMultigridBox(A, grid, 0.8, 2)
    check(L.psp_synchronize())
    t_create = time.perf_counter() - t
    info = K.info()
    out = {"grid": list(grid), "n": n, "nnz": nnz, "device": dev.device_info()[0], "levels": info["levels"],
           "tail_first_level": info["tail_first_level"], "launches_per_apply": info["launches_per_apply"],
           "operator": "Q1 Laplacian, constant coefficients, every entry of the box stored", "stencil": info["stencil"],
           "host_assembly_seconds": t_host, "handle_creation_seconds": t_create, "bytes": K.bytes()}
    out["bytes"]["operator_per_fine_point"] = out["bytes"]["operator"] / n
    bb, xb = dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    fill_random(L, check, bb, n)
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    # the cycle of the box handle and of an axis handle on the Poisson operator of the same grid, alternating
    Ap = dev.DeviceCSR.poisson(*grid)
    Ka = dev.DeviceMultigrid(Ap, grid, 0.8, 2, galerkin=True)
    out["axis_handle_bytes"] = Ka.bytes()
    rounds = {"box": [], "axis": []}
    for rnd in range(2):
        for label, H in (("box", K), ("axis", Ka)):
            rounds[label].append(cycle_time(L, H, bb, xb))
            print(json.dumps({"grid": name, "cycle": label, **rounds[label][-1]}), flush=True)
    mb = model_bytes(info["dims"], info["tail_first_level"], 2, nd)
    ma = model_bytes_axis(info["dims"], info["tail_first_level"], 2, nd)
    tb = min(r["median_ms"] for r in rounds["box"])
    ta = min(r["median_ms"] for r in rounds["axis"])
    out["vcycle"] = {"box": rounds["box"], "axis_on_poisson": rounds["axis"], "box_model_bytes": mb, "axis_model_bytes": ma,
                     "box_model_bytes_per_fine_point": mb / n, "axis_model_bytes_per_fine_point": ma / n,
                     "box_GBps_model": mb / tb / 1e6, "axis_GBps_model": ma / ta / 1e6,
                     "box_fraction_of_stream_probe": mb / tb / 1e6 / probe, "axis_fraction_of_stream_probe": ma / ta / 1e6 / probe,
                     "time_ratio_box_over_axis": tb / ta, "byte_ratio_box_over_axis": mb / ma}
    del Ka, Ap
    # time to solution, alternating
    J = dev.DeviceJacobi(A)
    aop, jop, kop = dev._Op(A, "matvec"), dev._Op(J, "precon"), dev._Op(K, "precon")
    rb = dev.DeviceBuffer(n)
    chunk = 1 << 24
    solves = {"jacobi": [], "box_multigrid": []}
    for rnd in range(2):
        for label, op in (("jacobi", jop), ("box_multigrid", kop)):
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
    tm = [s["seconds"] for s in solves["box_multigrid"]]
    out["pcg_to_1e-8"] = {"jacobi": solves["jacobi"], "box_multigrid": solves["box_multigrid"],
                          "time_ratio_jacobi_over_multigrid": min(tj) / min(tm),
                          "time_ratio_spread": [min(tj) / max(tm), max(tj) / min(tm)],
                          "iteration_ratio_jacobi_over_multigrid": solves["jacobi"][0]["iter"] / solves["box_multigrid"][0]["iter"]}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_box_timing.json"))
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--grids", help="comma-separated subset of the grids; results are merged into --out")
    p.add_argument("--case", help="(internal) run one grid in this process and print its JSON record")
    a = p.parse_args()
    cases = QUICK if a.quick else CASES
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, cases[a.case][0])), flush=True)
        return 0
    res = {"quick": a.quick, "cases": {},
           "not_run": {"512^3": "the 27-point CSR form has 3.6e9 entries, more than 32-bit row pointers hold"}}
    if a.grids and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    for name, (grid, limit) in cases.items():
        if a.grids and name not in a.grids.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name]
        if a.quick:
            cmd.append("--quick")
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("mg_box_timing: %s ended with status %d; nothing further is started" % (name, r.returncode), flush=True)
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
