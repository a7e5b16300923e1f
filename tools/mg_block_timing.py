"""Timing of the block V-cycle of precon.multigrid (psp_mg_precon_block_dev)
-> profiles/mg_block_timing.json.

The yardstick is what the library did before: k single applications (psp_mg_precon_dev) in the same process.  Per grid
and mode (matrix-free on the Poisson operator; galerkin=True on section 9d's smooth-kappa operator, built by
tools/mg_galerkin_timing.py) and k in {2, 4, 8}:

1. One block cycle against k single cycles: device-event time, 5 windows of each, the two ALTERNATING (block, singles,
   block, ...) in one process after a warm-up; medians, and the spread (min, max) of both.  Beside the measured ratio
   stands the byte model: galerkin (coef + vec k) / ((coef + vec) k) with coef = the bytes of a cycle that are level
   operators and w, vec = the rest (tools/mg_galerkin_timing.py's model_bytes split in two); matrix-free 1.0 (nothing
   is shared but the launches).  psp_stream_probe (2 read + 1 write) runs in the same process.
2. --variants: the same block window for the sweep's column counts (PSP_MG_BLOCK_KC = 2, 4) through the tuning switch
   (the child runs with PSP_TUNING=1); records "kc2", "kc4".  Records of earlier runs in the profile are keyed
   "kcr<R>_kc<C>": they also swept the restriction's residual tiles per workgroup, R = 2 and 4 of which are gone from the
   library (R = 1 is what it does); they are kept as they were.
3. --pcg: psp_pcg_batch_dev against k psp_pcg_dev to 1e-8 with the Galerkin cycle, host clock around synchronised calls,
   the two alternating twice.

Every grid runs in a child process of its own under `timeout`; the first child that fails ends the run.

    python tools/mg_block_timing.py [--out profiles/mg_block_timing.json] [--quick] [--grids 128^3,256^3]
                                    [--variants] [--pcg]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mg_timing import window_ms  # noqa: E402
from mg_galerkin_timing import fill_random, smooth_operator  # noqa: E402

CASES = {"128^3": ((128, 128, 128), 300), "256^3": ((256, 256, 256), 500), "4096^2": ((4096, 4096), 500),
         "512^3": ((512, 512, 512), 1100)}
QUICK = {"32^3": ((32, 32, 32), 120), "96^2": ((96, 96), 120)}
KS = (2, 4, 8)
WINDOWS = 5


def split_model_bytes(dims, tail_first, steps, nd, galerkin):
    """(coefficient bytes, vector bytes) of one application by the models of DESIGN.md 9c / 9d: per level above the tail the
    first pass, the further sweeps, the restriction and the prolongation; a stored level reads C = 1 + lower arrays
    coefficient arrays per pass, and w in every pass but the restriction"""
    coef = vec = 0.0
    for l in range(tail_first):
        n, nc = float(np.prod(dims[l])), float(np.prod(dims[l + 1]))
        c = ((nd + 1) if l == 0 else (3 ** nd + 1) // 2) if galerkin else 0
        w = 1 if galerkin else 0
        sweeps = max(steps - 2, 0) + steps
        if steps >= 2:
            coef += 8 * (c + w) * n
            vec += 16 * n
        else:
            coef += 8 * w * n
            vec += 16 * n
        coef += sweeps * 8 * (c + w) * n + 8 * c * n
        vec += sweeps * 24 * n + (16 * n + 8 * nc) + (16 * n + 8 * nc)
    return coef, vec + 16.0 * float(np.prod(dims[tail_first]))


def alternating(L, block, singles, reps):
    """WINDOWS windows of each, alternating; ms per application of the block / of the k singles"""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))
    tb, ts = [], []
    for _ in range(WINDOWS):
        tb.append(window_ms(L, ev, block, reps))
        ts.append(window_ms(L, ev, singles, reps))
    for e in ev:
        L.psp_event_destroy(e)
    mb, ms = statistics.median(tb), statistics.median(ts)
    return {"block_ms": {"median": mb, "min": min(tb), "max": max(tb)},
            "singles_ms": {"median": ms, "min": min(ts), "max": max(ts)},
            "ratio_block_over_singles": mb / ms, "ratio_spread": [min(tb) / max(ts), max(tb) / min(ts)],
            "reps_per_window": reps, "windows": WINDOWS}


def block_window(L, K, k, n, xb, yb, min_total_s=0.25):
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))

    def block():
        K.precon_block_dev(k, xb.ptr, n, yb.ptr, n)

    block()
    first = window_ms(L, ev, block, 3)
    reps = max(3, int(np.ceil(min_total_s * 1e3 / WINDOWS / max(first, 1e-3))))
    t = [window_ms(L, ev, block, reps) for _ in range(WINDOWS)]
    for e in ev:
        L.psp_event_destroy(e)
    return {"median": statistics.median(t), "min": min(t), "max": max(t), "reps_per_window": reps}


def measure_mode(L, K, n, nd, galerkin, xb, yb, probe, variants):
    info = K.info()
    coef, vec = split_model_bytes(info["dims"], info["tail_first_level"], 2, nd, galerkin)
    out = {"launches_per_apply": info["launches_per_apply"], "model_coef_bytes_per_point": coef / n,
           "model_vec_bytes_per_point": vec / n, "k": {}}
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))
    for k in KS:
        def block():
            K.precon_block_dev(k, xb.ptr, n, yb.ptr, n)

        def singles():
            for c in range(k):
                K.precon_dev(xb.ptr + 8 * n * c, yb.ptr + 8 * n * c)

        block()
        singles()
        L.psp_synchronize()
        first = window_ms(L, ev, singles, 3)
        reps = max(3, int(np.ceil(0.25e3 / WINDOWS / max(first, 1e-3))))
        r = alternating(L, block, singles, reps)
        r["model_ratio"] = (coef + vec * k) / ((coef + vec) * k)
        r["block_GBps_model"] = (coef + vec * k) / r["block_ms"]["median"] / 1e6
        r["block_fraction_of_stream_probe"] = r["block_GBps_model"] / probe
        r["block_storage"] = K.block_info()
        if variants:
            r["variants"] = {}
            for kc in (2, 4):
                if k <= 2 and kc != 2:
                    continue
                os.environ["PSP_MG_BLOCK_KC"] = str(kc)
                r["variants"]["kc%d" % kc] = block_window(L, K, k, n, xb, yb)
            os.environ.pop("PSP_MG_BLOCK_KC")
        out["k"][str(k)] = r
        print(json.dumps({"galerkin": galerkin, "k": k, **{a: r[a] for a in ("ratio_block_over_singles", "ratio_spread",
                                                                              "model_ratio")},
                          "variants": {a: b["median"] for a, b in r.get("variants", {}).items()}}), flush=True)
    for e in ev:
        L.psp_event_destroy(e)
    K.block_reserve(0)
    return out


def measure_pcg(L, dev, A, K, n, xb, bb):
    """psp_pcg_batch_dev against k psp_pcg_dev, alternating twice; host clock around synchronised calls"""
    from pysparse_amd._capi import check
    aop, kop = dev._Op(A, "matvec"), dev._Op(K, "precon")
    out = {}
    for k in KS:
        info, it, rr = (C.c_int * k)(), (C.c_int * k)(), (C.c_double * k)()
        runs = {"batch": [], "singles": []}
        for rnd in range(2):
            check(L.psp_memset(xb.ptr, 0, 8 * n * k))
            check(L.psp_synchronize())
            t = time.perf_counter()
            check(L.psp_pcg_batch_dev(aop._h, kop._h, n, k, xb.ptr, n, bb.ptr, n, 1e-8, 1000, info, it, rr))
            check(L.psp_synchronize())
            runs["batch"].append({"seconds": time.perf_counter() - t, "info": list(info), "iter": list(it)})
            launches = dev.last_solve_info()[1]["launches"]
            check(L.psp_memset(xb.ptr, 0, 8 * n * k))
            check(L.psp_synchronize())
            i1, it1, rr1 = C.c_int(), C.c_int(), C.c_double()
            its = []
            t = time.perf_counter()
            for c in range(k):
                check(L.psp_pcg_dev(aop._h, kop._h, n, xb.ptr + 8 * n * c, bb.ptr + 8 * n * c, 1e-8, 1000, C.byref(i1),
                                    C.byref(it1), C.byref(rr1), None))
                its.append(it1.value)
            check(L.psp_synchronize())
            runs["singles"].append({"seconds": time.perf_counter() - t, "iter": its})
        tb = [r["seconds"] for r in runs["batch"]]
        ts = [r["seconds"] for r in runs["singles"]]
        out[str(k)] = {**runs, "launches_per_iteration": launches, "ratio_batch_over_singles": min(tb) / min(ts),
                       "ratio_spread": [min(tb) / max(ts), max(tb) / min(ts)]}
        print(json.dumps({"pcg_k": k, "batch_s": tb, "singles_s": ts, "iter": runs["batch"][0]["iter"]}), flush=True)
    return out


def run_case(name, grid, variants, pcg):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    nd, n = len(grid), int(np.prod(grid))
    kmax = max(KS)
    out = {"grid": list(grid), "n": n, "device": dev.device_info()[0]}
    xb, yb = dev.DeviceBuffer(n * kmax), dev.DeviceBuffer(n * kmax)
    fill_random(L, check, xb, n * kmax)
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    probe = 3.0 * stream_bytes / avg.value / 1e6
    out["stream_probe_2r1w"] = {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value, "GBps": probe}
    Ac = dev.DeviceCSR.poisson(*grid)
    Km = dev.DeviceMultigrid(Ac, grid, 0.8, 2)
    out["matrix_free"] = measure_mode(L, Km, n, nd, False, xb, yb, probe, variants)
    del Km, Ac
    ind, col, val = smooth_operator(grid)
    A = dev.DeviceCSR.from_arrays((n, n), ind, col, val)
    del ind, col, val
    Kg = dev.DeviceMultigrid(A, grid, 0.8, 2, galerkin=True)
    out["galerkin"] = measure_mode(L, Kg, n, nd, True, xb, yb, probe, variants)
    if pcg:
        out["pcg_to_1e-8_galerkin"] = measure_pcg(L, dev, A, Kg, n, yb, xb)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_block_timing.json"))
    p.add_argument("--quick", action="store_true", help="two small grids: a rehearsal of the tool, not a measurement")
    p.add_argument("--grids", help="comma-separated subset of the grids; results are merged into --out")
    p.add_argument("--variants", action="store_true", help="also time the sweep's column counts (KC = 2, 4)")
    p.add_argument("--pcg", action="store_true", help="also time psp_pcg_batch_dev against k psp_pcg_dev")
    p.add_argument("--case", help="(internal) run one grid in this process and print its JSON record")
    a = p.parse_args()
    cases = QUICK if a.quick else CASES
    if a.case:
        print("RESULT " + json.dumps(run_case(a.case, cases[a.case][0], a.variants, a.pcg)), flush=True)
        return 0
    res = {"quick": a.quick, "cases": {}}
    if a.grids and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    env = dict(os.environ)
    if a.variants:
        env["PSP_TUNING"] = "1"
    for name, (grid, limit) in cases.items():
        if a.grids and name not in a.grids.split(","):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--case", name]
        cmd += ["--quick"] * a.quick + ["--variants"] * a.variants + ["--pcg"] * a.pcg
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("mg_block_timing: %s ended with status %d; nothing further is started" % (name, r.returncode), flush=True)
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
