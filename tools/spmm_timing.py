#!/usr/bin/env python3
"""Timing of the block products and the batched PCG loop (psp_spmm.hip, psp_batch.hip) -> profiles/spmm_timing.json.
Run by hand on the GPU; no test reads the result.

1. Products.  psp_csr_matmat_dev / psp_sss_matmat_dev at k = 1, 2, 4, 8, 16 against k calls of the single-vector
   psp_csr_matvec_dev / psp_sss_matvec_dev on the same handle in the same process, alternating inside every window:
     * 512^3 Poisson in the index-free layout (psp_csr_poisson_big; csr_spmm_w4 against csr_spmv_w4);
     * the FEM stand-in (pysparse_amd/tools/standins.py, n = 929 424, 45 entries per row) as an sss_mat, whose block
       product is csr_spmm_rows on the expanded mirror -- once on a fresh handle (single products: the stored numbering)
       and once on a handle that was told to expect many products (single products: the renumbered copy).
   Beside them psp_stream_probe with 7 reads + 1 write of 1 GiB: what a plain streaming kernel gets in this process.
2. Solves.  psp_pcg_batch_dev at k = 4 and 8 against k sequential psp_pcg_dev (jacobi, 40 iterations, device vectors on
   both sides) at 256^3 and 4096^2.

Method: every figure is the median over `windows` windows of device-event time (products) or host wall time around calls
that end synchronised (solves), each window after the warm-up holding `reps` calls; min and max of the windows are kept as
the spread.  The two sides of a comparison alternate window by window.

    python tools/spmm_timing.py [--out profiles/spmm_timing.json] [--quick]
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

KS = (1, 2, 4, 8, 16)


def window_ms(L, ev, fn, reps):
    L.psp_event_record(ev[0])
    for _ in range(reps):
        fn()
    L.psp_event_record(ev[1])
    ms = C.c_float()
    L.psp_event_elapsed_ms(ev[0], ev[1], C.byref(ms))
    return ms.value / reps


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def products(L, dev, A, nrows, matrix_bytes_per_row, reps, windows, label):
    """block product against k single products, alternating; returns one row per k"""
    kmax = max(KS)
    x = np.random.default_rng(0).standard_normal(nrows)
    dX, dY = dev.DeviceBuffer(nrows * kmax), dev.DeviceBuffer(nrows * kmax)
    for c in range(kmax):
        L.psp_memcpy_h2d(dX.ptr + 8 * nrows * c, x.ctypes.data, 8 * nrows)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))
    rows = []
    for k in KS:
        def block():
            A.matmat_dev(k, dX.ptr, nrows, dY.ptr, nrows)

        def singles():
            for c in range(k):
                A.matvec_dev(dX.ptr + 8 * nrows * c, dY.ptr + 8 * nrows * c)

        kernel_before = A.kernel_info()[0]
        for _ in range(2):
            block()
            singles()
        L.psp_synchronize()
        tb, ts = [], []
        for _ in range(windows):
            ts.append(window_ms(L, ev, singles, reps))
            tb.append(window_ms(L, ev, block, reps))
        sb, ss = stats(tb), stats(ts)
        model = (matrix_bytes_per_row + 16.0 * k) / (k * (matrix_bytes_per_row + 16.0))
        rows.append({"matrix": label, "k": k, "single_kernel": kernel_before, "single_kernel_after": A.kernel_info()[0],
                     "block": sb, "k_singles": ss, "ratio_block_over_singles": sb["median_ms"] / ss["median_ms"],
                     "singles_spread_rel": (ss["max_ms"] - ss["min_ms"]) / ss["median_ms"],
                     "byte_model_ratio": model,
                     "block_GBps_model": (matrix_bytes_per_row + 16.0 * k) * nrows / sb["median_ms"] / 1e6})
        print(json.dumps(rows[-1]), flush=True)
    for e in ev:
        L.psp_event_destroy(e)
    dX.free()
    dY.free()
    return rows


def solves(L, dev, grid, reps, windows):
    """device vectors on both sides, so that the loops are timed and not the host copies"""
    from pysparse_amd._capi import check
    A = dev.DeviceCSR.poisson(*grid)
    n = A.shape[0]
    K = dev.DeviceJacobi(A, 1.0, 1)
    aop, kop = dev._Op(A, "matvec"), dev._Op(K, "precon")
    rng = np.random.default_rng(1)
    rows = []
    for k in (4, 8):
        dB, dX = dev.DeviceBuffer(n * k), dev.DeviceBuffer(n * k)
        for c in range(k):
            b = rng.standard_normal(n)
            L.psp_memcpy_h2d(dB.ptr + 8 * n * c, b.ctypes.data, 8 * n)
        info, it, rr = (C.c_int * k)(), (C.c_int * k)(), (C.c_double * k)()

        def batch():
            dX.zero()
            check(L.psp_pcg_batch_dev(aop._h, kop._h, n, k, dX.ptr, n, dB.ptr, n, 1e-30, 40, info, it, rr))

        def singles():
            dX.zero()
            for c in range(k):
                i1, t1, r1 = C.c_int(), C.c_int(), C.c_double()
                check(L.psp_pcg_dev(aop._h, kop._h, n, dX.ptr + 8 * n * c, dB.ptr + 8 * n * c, 1e-30, 40, C.byref(i1),
                                    C.byref(t1), C.byref(r1), None))

        batch()
        loop_batch = dev.last_solve_info()
        xb = dX.download()
        singles()
        loop_single = dev.last_solve_info()
        same = bool(np.array_equal(xb, dX.download()))
        tb, ts = [], []
        for _ in range(windows):
            for fn, acc in ((singles, ts), (batch, tb)):
                L.psp_synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                L.psp_synchronize()
                acc.append((time.perf_counter() - t0) * 1e3 / reps)
        sb, ss = stats(tb), stats(ts)
        rows.append({"grid": list(grid), "n": n, "k": k, "iterations": 40, "batch_loop": loop_batch[0],
                     "batch_launches_per_iteration": loop_batch[1]["launches"], "single_loop": loop_single[0],
                     "x_bit_identical": same, "batch": sb, "k_singles": ss,
                     "ratio_batch_over_singles": sb["median_ms"] / ss["median_ms"],
                     "singles_spread_rel": (ss["max_ms"] - ss["min_ms"]) / ss["median_ms"]})
        print(json.dumps(rows[-1]), flush=True)
        dB.free()
        dX.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_timing.json"))
    ap.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    from pysparse_amd.tools.standins import fem_sss_arrays
    L = lib()
    res = {"device": dev.device_info()[0], "quick": a.quick, "products": [], "solves": []}
    avg, mn = C.c_float(), C.c_float()
    nbytes = (1 << 24) if a.quick else (1 << 30)
    check(L.psp_stream_probe(7, 1, C.c_size_t(nbytes), 10, C.byref(avg), C.byref(mn)))
    res["stream_probe_7r1w"] = {"bytes_per_stream": nbytes, "avg_ms": avg.value, "min_ms": mn.value,
                                "GBps": 8.0 * nbytes / mn.value / 1e6}
    print(json.dumps(res["stream_probe_7r1w"]), flush=True)
    g = (64, 64, 64) if a.quick else (512, 512, 512)
    A = dev.DeviceCSR.poisson_big(*g)
    res["products"] += products(L, dev, A, A.shape[0], 58.0, 10, 5, "poisson_big %dx%dx%d (csr_spmm_w4)" % g)
    A.close()
    L.psp_trim()
    fg = (16, 16, 16) if a.quick else (68, 68, 67)
    n, ind, col, val, diag = fem_sss_arrays(*fg)
    per_row = 12.0 * (2 * len(col) + n) / n + 4.0
    S = dev.DeviceSSS.from_arrays(n, ind, col, val, diag)
    res["products"] += products(L, dev, S, n, per_row, 5, 5, "fem stand-in %dx%dx%d, fresh handle (csr_spmm_rows)" % fg)
    S.close()
    S = dev.DeviceSSS.from_arrays(n, ind, col, val, diag)
    S.prepare(1 << 30)
    res["products"] += products(L, dev, S, n, per_row, 10, 5,
                                "fem stand-in %dx%dx%d, prepared handle (csr_spmm_rows)" % fg)
    S.close()
    L.psp_trim()
    for grid in (((32, 32, 32), (128, 128, 0)) if a.quick else ((256, 256, 256), (4096, 4096, 0))):
        res["solves"] += solves(L, dev, grid, 2, 3)
        L.psp_trim()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
