"""Timing of the block kernels and of the solver of pysparse.eigen.lobpcg
-> profiles/lobpcg_timing.json.  Protocol of sections 9c / 9e: medians of 5 windows, the contenders ALTERNATING window by
window in one process after a warm-up, psp_stream_probe (2 read + 1 write) in the same process, the spread (min, max)
beside every median.

(a) --gram: psp_bv_gram against what the library did before it, mb calls of psp_bv_tdot, at n = 2^24 and
    (ma, mb) in {(4,4), (8,8), (12,12), (24,24)}: device-event time.  Beside the ratio stands the byte model
    8 n (ma ceil(mb/4) + mb ceil(ma/8)) against 8 n mb (ma + 1).
(b) --solve: time to k in {4, 8} eigenpairs at tol 1e-8 on the 256^3 Poisson operator with precon.multigrid as K:
    psp_lobpcg against psp_jdsym (kmax = k, tau = 0, the given inner solvers, the same K), host clock around the
    synchronous C entry points (both copy their vectors to the host inside the call), with the iteration counts -- for
    lobpcg one block product and one block cycle per iteration -- and the residuals recomputed through A.matvec.

Each part runs in a child process of its own under `timeout`; a child that fails ends the run.

    python tools/lobpcg_timing.py [--out profiles/lobpcg_timing.json] [--gram] [--solve] [--quick] [--windows 5]
                                  [--inner qmrs,pcg]
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

SHAPES = ((4, 4), (8, 8), (12, 12), (24, 24))
TA, TB = 8, 4


def stream_probe(L, check, n):
    stream_bytes = max(4096, (8 * n) // 4096 * 4096)
    avg, mn = C.c_float(), C.c_float()
    check(L.psp_stream_probe(2, 1, C.c_size_t(stream_bytes), 10, C.byref(avg), C.byref(mn)))
    return {"bytes_per_stream": stream_bytes, "avg_ms": avg.value, "min_ms": mn.value,
            "GBps": 3.0 * stream_bytes / avg.value / 1e6}


def summary(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def run_gram(n, windows):
    from pysparse_amd import device as dev
    from pysparse_amd._capi import check, lib
    L = lib()
    mmax = max(max(s) for s in SHAPES)
    out = {"n": n, "device": dev.device_info()[0], "stream_probe_2r1w": stream_probe(L, check, n), "shapes": {}}
    A, B, G = dev.DeviceBuffer(n * mmax), dev.DeviceBuffer(n * mmax), dev.DeviceBuffer(mmax * mmax)
    v = np.random.default_rng(0).standard_normal(n)
    w = v[::-1].copy()  # kept alive by name: the calls below take bare addresses
    for c in range(mmax):  # the values do not matter to the time: one column of noise, copied
        check(L.psp_memcpy_h2d(A.ptr + 8 * n * c, v.ctypes.data, 8 * n))
        check(L.psp_memcpy_h2d(B.ptr + 8 * n * c, w.ctypes.data, 8 * n))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        L.psp_event_create(C.byref(e))
    for ma, mb in SHAPES:
        def gram():
            check(L.psp_bv_gram(n, ma, A.ptr, n, mb, B.ptr, n, G.ptr, ma))

        def tdots():
            for b in range(mb):
                check(L.psp_bv_tdot(n, ma, A.ptr, n, B.ptr + 8 * n * b, G.ptr + 8 * ma * b))

        gram()
        g1 = G.download()[:ma * mb].copy()
        tdots()
        same = bool(np.array_equal(g1, G.download()[:ma * mb]))
        L.psp_synchronize()
        first = window_ms(L, ev, tdots, 2)
        reps = max(2, int(np.ceil(0.25e3 / windows / max(first, 1e-3))))
        tg, tt = [], []
        for _ in range(windows):
            tg.append(window_ms(L, ev, gram, reps))
            tt.append(window_ms(L, ev, tdots, reps))
        bg = 8.0 * n * (ma * -(-mb // TB) + mb * -(-ma // TA))
        bt = 8.0 * n * mb * (ma + 1)
        r = {"gram_ms": summary(tg), "tdots_ms": summary(tt), "ratio_gram_over_tdots": statistics.median(tg) / statistics.median(tt),
             "ratio_spread": [min(tg) / max(tt), max(tg) / min(tt)], "model_ratio": bg / bt,
             "gram_GBps_model": bg / statistics.median(tg) / 1e6, "tdots_GBps_model": bt / statistics.median(tt) / 1e6,
             "bits_equal_to_tdot": same, "reps_per_window": reps, "windows": windows}
        out["shapes"]["%dx%d" % (ma, mb)] = r
        print(json.dumps({"shape": [ma, mb], **{a: r[a] for a in ("ratio_gram_over_tdots", "ratio_spread", "model_ratio",
                                                                  "bits_equal_to_tdot")}}), flush=True)
    for e in ev:
        L.psp_event_destroy(e)
    return out


def run_solve(grid, ks, windows, inners):
    from pysparse_amd import _capi, device as dev
    from pysparse_amd._capi import check, lib
    from pysparse_amd.eigen._operands import _Operator
    from pysparse.precon import precon
    from pysparse.sparse import spmatrix
    L = lib()
    n = int(np.prod(grid))
    A = spmatrix.poisson_csr(*grid)
    K = precon.multigrid(A, grid)
    opA, opK = _Operator(A, n, False), _Operator(K, n, True)
    out = {"grid": list(grid), "n": n, "tol": 1e-8, "device": dev.device_info()[0],
           "stream_probe_2r1w": stream_probe(L, check, n), "k": {}}
    lin = {"pcg": _capi.LIN_PCG, "qmrs": _capi.LIN_QMRS}
    spectrum = np.zeros(1)
    for m in grid:
        spectrum = np.sort((spectrum[:, None] + (2.0 - 2.0 * np.cos(np.pi * np.arange(1, 12) / (m + 1)))[None, :]).ravel())[:64]

    def true_residuals(lam, Q):  # Q: (k, n) rows = vectors
        y = np.empty(n)
        res = []
        for lm, q in zip(lam, Q):
            A.matvec(q, y)
            res.append(float(np.linalg.norm(y - lm * q)))
        return res

    for k in ks:
        lam, res, Q = np.zeros(k), np.zeros(k), np.zeros((k, n))
        kconv, it, it_in = C.c_int(), C.c_int(), C.c_int()

        def lobpcg():
            t = time.perf_counter()
            check(L.psp_lobpcg(opA.ptr, None, opK.ptr, n, k, 1e-8, 500, None, 0, 0, lam.ctypes.data, Q.ctypes.data, n,
                               res.ctypes.data, C.byref(kconv), C.byref(it)))
            return time.perf_counter() - t

        def jdsym(code):
            p = _capi.JdsymParams()
            p.kmax, p.jmax, p.jmin, p.itmax, p.blksize, p.blkwise = k, 25, 10, 500, 1, 0
            p.optype, p.linitmax, p.strategy, p.clvl = 2, 200, 0, 0
            p.tau, p.jdtol, p.eps_tr, p.toldecay, p.linsolver = 0.0, 1e-8, 1e-3, 1.5, code
            t = time.perf_counter()
            check(L.psp_jdsym(opA.ptr, None, opK.ptr, n, C.byref(p), C.byref(kconv), lam.ctypes.data, Q.ctypes.data,
                              C.byref(it), C.byref(it_in)))
            return time.perf_counter() - t

        rec = {"lobpcg": {"seconds": []}}
        for name in inners:
            rec["jdsym_" + name] = {"seconds": []}
        for w in range(windows + 1):  # the first round is the warm-up (allocations, level vectors)
            s = lobpcg()
            if w > 0:
                rec["lobpcg"]["seconds"].append(s)
            rec["lobpcg"].update(iterations=it.value, block_products=it.value, block_cycles=it.value, kconv=kconv.value,
                                 eigenvalue_error=float(np.abs(lam - spectrum[:k]).max()))
            if w == windows:
                rec["lobpcg"]["true_residuals"] = true_residuals(lam, Q)
            for name in inners:
                s = jdsym(lin[name])
                r = rec["jdsym_" + name]
                if w > 0:
                    r["seconds"].append(s)
                r.update(outer_iterations=it.value, inner_iterations=it_in.value, kconv=kconv.value,
                         eigenvalue_error=float(np.abs(np.sort(lam[:kconv.value]) - spectrum[:kconv.value]).max())
                         if kconv.value else None)
                if w == windows:
                    r["true_residuals"] = true_residuals(lam[:kconv.value], Q[:kconv.value])
        for r in rec.values():
            r["seconds_summary"] = summary(r["seconds"])
        tl = rec["lobpcg"]["seconds"]
        for name in inners:
            tj = rec["jdsym_" + name]["seconds"]
            rec["ratio_lobpcg_over_jdsym_" + name] = {"median": statistics.median(tl) / statistics.median(tj),
                                                     "spread": [min(tl) / max(tj), max(tl) / min(tj)]}
        rec["windows"] = windows
        out["k"][str(k)] = rec
        print(json.dumps({"k": k, **{a: (b["seconds_summary"]["median"] if isinstance(b, dict) and "seconds_summary" in b
                                        else b) for a, b in rec.items()}}), flush=True)
    opA.close()
    opK.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lobpcg_timing.json"))
    p.add_argument("--gram", action="store_true")
    p.add_argument("--solve", action="store_true")
    p.add_argument("--quick", action="store_true", help="small sizes: a rehearsal of the tool, not a measurement")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--inner", default="qmrs,pcg")
    p.add_argument("--part", help="(internal) run one part in this process and print its JSON record")
    a = p.parse_args()
    inners = [s for s in a.inner.split(",") if s]
    if a.part == "gram":
        print("RESULT " + json.dumps(run_gram(1 << (18 if a.quick else 24), a.windows)), flush=True)
        return 0
    if a.part == "solve":
        grid = (32, 32, 32) if a.quick else (256, 256, 256)
        print("RESULT " + json.dumps(run_solve(grid, (4, 8), a.windows, inners)), flush=True)
        return 0
    res = {"quick": a.quick}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if old.get("quick") == a.quick:
            res = old
    for part, limit in (("gram", 400), ("solve", 1000)):
        if not getattr(a, part) and (a.gram or a.solve):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--windows", str(a.windows), "--inner", a.inner] + ["--quick"] * a.quick
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        lines = []
        for ln in proc.stdout:  # passed on as it comes: a long part is seen to be alive
            if not ln.startswith("RESULT "):
                sys.stdout.write(ln)
                sys.stdout.flush()
            lines.append(ln)
        rc = proc.wait()
        if rc != 0:
            print("lobpcg_timing: %s ended with status %d; nothing further is started" % (part, rc), flush=True)
            return 1
        line = [ln for ln in lines if ln.startswith("RESULT ")][-1]
        res[part] = json.loads(line[len("RESULT "):])
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
