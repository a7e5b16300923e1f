"""Timing of precon.multigrid (pysparse_amd/csrc/psp_mg.hip) -> profiles/mg_timing.json.

Per grid (256^3, 512^3, 4096^2, and 128^3 for the tail's share), on the Poisson operator in the index-free layout:

1. One V-cycle (psp_mg_precon_dev, omega 0.8, steps 2): device-event time per application after a warm-up, median of
   windows that together hold at least 0.5 s of work; the cycle's bytes from the byte model of DESIGN.md section 9c
   (model_bytes below, computed from the level sizes); that rate over the same process's psp_stream_probe with the
   smoother's access shape (2 read streams + 1 write stream of the fine level's size).
2. Time to solution: psp_pcg_dev to 1e-8 on a seeded random right-hand side, device vectors on both sides, host clock around
   calls that end synchronised -- precon.jacobi and precon.multigrid alternating in one process, iteration counts and the
   true relative residual of each.
3. 128^3 only: the single-workgroup tail launch's share of a cycle, measured as the one-launch application of a handle
   whose whole grid is the tail's first level.

Every grid runs in a child process of its own under `timeout`; the first child that fails ends the run.

--precision single measures the float32 cycle of DESIGN.md section 9g (device.DeviceMultigrid32) with that section's byte
model; the default output file then is profiles/mg_timing_single.json.

    python tools/mg_timing.py [--out profiles/mg_timing.json] [--quick] [--precision double|single]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"128^3": ((128, 128, 128), 300), "256^3": ((256, 256, 256), 400), "512^3": ((512, 512, 512), 900),
         "4096^2": ((4096, 4096), 600)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}


def model_bytes(dims, tail_first, steps, single=False):
    """bytes one application moves through memory by the kernels' own reads and writes (neighbours come from the caches):
    per level above the tail the pre-smoothing (first pass: read b, write x; 24 B per point and further sweep), the
    restriction (read x and b, write b_c), the prolongation (read x and e, write x) and `steps` sweeps of 24 B; the tail reads
    its b and writes its x once.  single: every level vector is 4 B per point; the finest level's b stays
    the caller's 8 B wherever it is read, and its last sweep writes the caller's 8 B"""
    e = 4 if single else 8
    total = 0.0
    for l in range(tail_first):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        eb = 8 if l == 0 else e
        sweep = 2 * e + eb
        total += n * ((eb + e) + sweep * max(steps - 2, 0)) + ((e + eb) * n + e * nc) + (2 * e * n + e * nc) + sweep * steps * n
        if l == 0:
            total += (8 - e) * n
    return total + (16.0 if tail_first == 0 else 2.0 * e) * float(np.prod(dims[tail_first]))


def window_ms(L, ev, fn, reps):
    L.psp_event_record(ev[0])
    for _ in range(reps):
        fn()
    L.psp_event_record(ev[1])
    ms = C.c_float()
    L.psp_event_elapsed_ms(ev[0], ev[1], C.byref(ms))
    return ms.value / reps


def cycle_time(L, K, xb, yb, min_total_s=0.5, windows=5):
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))

    def once():
        K.precon_dev(xb.ptr, yb.ptr)

    for _ in range(3):
        once()
    L.psp_synchronize()
    first = window_ms(L, ev, once, 5)
    reps = max(5, int(np.ceil(min_total_s * 1e3 / windows / max(first, 1e-3))))
    t = [window_ms(L, ev, once, reps) for _ in range(windows)]
    for e in ev:
        L.psp_event_destroy(e)
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "reps_per_window": reps,
            "windows": windows}


def run_case(name, grid, precision="double"):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    n = int(np.prod(grid))
    single = precision == "single"
    Multigrid = dev.DeviceMultigrid32 if single else dev.DeviceMultigrid
    A = dev.DeviceCSR.poisson_big(*grid)
    K = Multigrid(A, grid, 0.8, 2)
    J = dev.DeviceJacobi(A)
    info = K.info()
    out = {"grid": list(grid), "n": n, "device": dev.device_info()[0], "levels": info["levels"],
           "tail_first_level": info["tail_first_level"], "launches_per_apply": info["launches_per_apply"],
           "precision": info["precision"], "bytes": K.bytes()}
    bb, xb = dev.DeviceBuffer(n), dev.DeviceBuffer(n)
    g = np.random.default_rng(0)
    chunk = 1 << 24
    for k in range(0, n, chunk):
        v = g.standard_normal(min(chunk, n - k))
        check(L.psp_memcpy_h2d(bb.ptr + 8 * k, v.ctypes.data, 8 * v.size))
    # 1. the cycle
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    cyc = cycle_time(L, K, bb, xb)
    mb = model_bytes(info["dims"], info["tail_first_level"], 2, single)
    cyc.update({"model_bytes": mb, "model_bytes_per_fine_point": mb / n, "GBps_model": mb / cyc["median_ms"] / 1e6,
                "fraction_of_stream_probe": mb / cyc["median_ms"] / 1e6 / probe})
    out["vcycle"] = cyc
    print(json.dumps({"grid": name, "vcycle": cyc}), flush=True)
    if name == "128^3" or name in QUICK:
        tg = info["dims"][info["tail_first_level"]]
        tgrid = tuple(d for d in tg if d > 1) or (1,)
        nt = int(np.prod(tgrid))
        At = dev.DeviceCSR.poisson_big(*tgrid) if len(tgrid) > 1 else None
        if At is not None:
            Kt = Multigrid(At, tgrid, 0.8, 2)
            tb, tx = dev.DeviceBuffer.from_host(np.ones(nt)), dev.DeviceBuffer(nt)
            tail = cycle_time(L, Kt, tb, tx, min_total_s=0.2)
            tail["grid"] = list(tgrid)
            tail["share_of_cycle"] = tail["median_ms"] / cyc["median_ms"]
            out["tail_launch"] = tail
    # 2. time to solution, alternating
    aop, jop, kop = dev._Op(A, "matvec"), dev._Op(J, "precon"), dev._Op(K, "precon")
    rb = dev.DeviceBuffer(n)
    solves = {"jacobi": [], "multigrid": []}
    for rnd in range(2):
        for label, op in (("jacobi", jop), ("multigrid", kop)):
            xb.zero()
            i, it, rr = C.c_int(), C.c_int(), C.c_double()
            check(L.psp_synchronize())
            t = time.perf_counter()
            check(L.psp_pcg_dev(aop._h, op._h, n, xb.ptr, bb.ptr, 1e-8, 100000, C.byref(i), C.byref(it), C.byref(rr), None))
            check(L.psp_synchronize())
            dt = time.perf_counter() - t
            # the true residual ||b - A x|| / ||b||
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
    tj = min(s["seconds"] for s in solves["jacobi"])
    tm = min(s["seconds"] for s in solves["multigrid"])
    out["pcg_to_1e-8"] = {"jacobi": solves["jacobi"], "multigrid": solves["multigrid"],
                          "time_ratio_jacobi_over_multigrid": tj / tm,
                          "iteration_ratio_jacobi_over_multigrid": solves["jacobi"][0]["iter"] / solves["multigrid"][0]["iter"]}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out")
    p.add_argument("--precision", choices=["double", "single"], default="double")
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--case", help="(internal) run one grid in this process and print its JSON record")
    a = p.parse_args()
    if not a.out:
        a.out = os.path.join(ROOT, "profiles", "mg_timing.json" if a.precision == "double" else "mg_timing_single.json")
    cases = QUICK if a.quick else CASES
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, cases[a.case][0], a.precision)), flush=True)
        return 0
    res = {"quick": a.quick, "precision": a.precision, "cases": {}}
    for name, (grid, limit) in cases.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name,
               "--precision", a.precision]
        if a.quick:
            cmd.append("--quick")
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("mg_timing: %s ended with status %d; nothing further is started" % (name, r.returncode), flush=True)
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
