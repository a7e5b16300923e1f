"""Plain NumPy statements of the fused vector passes of pysparse_amd/csrc/psp_vec.hip that psp_debug_vec_pass launches.

Each function is written from the reference loop it replaces (bicgstab.c, cgs.c, qmrs.c, gmres.c, minres.c,
preconmodule.c) and the comment above its kernel, one rounded operation at a time -- `1.0 * x + a * y` where the library
goes through lin2, the copy + daxpy pairs of cgs.c with netlib daxpy's quick return for a zero coefficient.  The passes are
element-wise and the library is built without FMA contraction, so these expressions give the kernels' vectors bit for bit.

    f(v, s, dinv=None, **form) -> (out, sums)

v: {name: array} of the pass's vectors (never modified), s: its scalars in the order of include/pysparse_hip.h, dinv: the
Jacobi array or None.  out: {name: new array} of every vector the pass writes; sums: the reductions as (a, b) pairs whose
sum of products the pass leaves.  tests/test_vec_passes_host.py composes them into the solvers' loops and compares with
the oracle; tests/test_gpu_vec_passes.py compares each kernel with them.

PASSES gives per pass what the kernel -- not its launch wrapper -- dereferences 16 bytes at a time: `always` in every form,
`with_pre` only with a preconditioner, `dinv` whether the array form reads dinv ('always': in every form)."""
import numpy as np


def _K(t, dinv):
    return t if dinv is None else t * dinv


def lin2(v, s, dinv=None):
    a, b = s
    return {"z": a * v["x"] + b * v["y"]}, []


def scal(v, s, dinv=None):
    return {"x": s[0] * v["x"]}, []


def bicg_p(v, s, dinv=None, first=False):
    """bicgstab.c:250-261: p = r (iteration 1) or r + beta (p - omega v); phat = K p"""
    beta, omega = s
    if first:
        p = v["r"].copy()
    else:
        t = 1.0 * v["p"] + (-omega) * v["v"]
        p = 1.0 * v["r"] + beta * t
    out = {"p": p}
    if dinv is not None:
        out["phat"] = p * dinv
    return out, []


def bicg_s(v, s, dinv=None):
    """bicgstab.c:265-271: s = r + (-alpha) v; shat = K s"""
    sv = 1.0 * v["r"] + (-s[0]) * v["v"]
    out = {"s": sv}
    if dinv is not None:
        out["shat"] = sv * dinv
    return out, []


def bicg_xr(v, s, dinv=None):
    """bicgstab.c:275-278 and :247 of the next iteration"""
    alpha, omega = s
    x = 1.0 * v["x"] + alpha * v["phat"]
    x = 1.0 * x + omega * v["shat"]
    r = 1.0 * v["s"] + (-omega) * v["t"]
    return {"x": x, "r": r}, [(r, r), (v["rhat"], r)]


def cgs_q(v, s, dinv=None):
    """cgs.c:74-84"""
    alpha = s[0]
    q = 1.0 * v["u"] + (-alpha) * v["v"] if alpha != 0.0 else v["u"].copy()
    t = 1.0 * v["u"] + 1.0 * q
    tmp2 = _K(t, dinv)
    x = 1.0 * v["x"] + alpha * tmp2 if alpha != 0.0 else v["x"].copy()
    return {"q": q, "tmp2": tmp2, "x": x}, []


def cgs_r(v, s, dinv=None):
    """cgs.c:87-95"""
    alpha = s[0]
    r = 1.0 * v["r"] + (-alpha) * v["t"] if alpha != 0.0 else v["r"].copy()
    return {"r": r}, [(r, r), (r, v["r0"])]


def cgs_p(v, s, dinv=None):
    """cgs.c:99-105 and :66-67 of the next iteration"""
    beta = s[0]
    if beta != 0.0:
        u = 1.0 * v["r"] + beta * v["q"]
        t = 1.0 * v["q"] + beta * v["p"]
        p = 1.0 * u + beta * t
    else:
        u = v["r"].copy()
        p = u.copy()
    out = {"u": u, "p": p}
    if dinv is not None:
        out["kp"] = p * dinv
    return out, []


def qmrs_kv(v, s, dinv=None):
    """qmrs.c:91-95"""
    if dinv is None:
        return {}, [(v["v1"], v["v1"])]
    w = v["v1"] * dinv
    return {"wrk1": w}, [(w, v["v1"])]


def qmrs_pg(v, s, dinv=None):
    """qmrs.c:101-104"""
    cc = s[0]
    return {"p": 1.0 * v["v1"] + (-cc) * v["p"], "g": 1.0 * v["wrk1"] + (-cc) * v["g"]}, []


def qmrs_v(v, s, dinv=None):
    """qmrs.c:108-111"""
    v1 = 1.0 * v["t"] + (-s[0]) * v["v1"]
    return {"v1": v1}, [(v1, v1)]


def qmrs_dx(v, s, dinv=None):
    """qmrs.c:130-134 and :91-95 of the next iteration"""
    eta, cc, rho1inv = s
    d = eta * v["p"] + cc * v["d"]
    x = 1.0 * v["x"] + 1.0 * d
    v1 = rho1inv * v["v1"]
    out = {"d": d, "x": x, "v1": v1}
    w = v1
    if dinv is not None:
        w = out["wrk1"] = v1 * dinv
    return out, [(w, v1)]


def axpy_dot(v, s, dinv=None):
    """gmres.c:143-145: the daxpy of one Gram-Schmidt step and the inner product of the next (z None: the norm's square)"""
    a = s[0]
    y = 1.0 * v["y"] + a * v["x"] if a != 0.0 else v["y"].copy()
    return {"y": y}, [(y, y if v.get("z") is None else v["z"])]


def axpy_dot_chain(v, s, dinv=None, h=None):
    """the same step with its coefficient -h, h the sum the step before left in partial sums (given here)"""
    return axpy_dot(v, [-h])


def jacobi_sweep(v, s, dinv=None):
    """preconmodule.c:50-51"""
    return {"y": (v["x"] - v["y"]) * dinv + v["temp"]}, []


def dinv(v, s, dinv=None):
    """preconmodule.c:395-400; the 'sum' is the number of entries with 1 + d == 1"""
    d = v["diag"]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = s[0] / d
    sing = (1.0 + d == 1.0).astype(np.float64)
    return {"dinv": out}, [(sing, np.ones_like(d))]


def scale_div(v, s, dinv=None):
    """minres.c:123-124"""
    return {"v": v["y"] / s[0]}, []


def lanczos(v, s, dinv=None):
    """minres.c:131-143; the new v_hat is written over v_hat_old"""
    c1, c2 = s
    nv = v["av"] - c1 * v["v_hat"] - c2 * v["v_hat_old"]
    if dinv is None:
        return {"v_hat_old": nv}, [(nv, nv)]
    y = nv * dinv
    return {"v_hat_old": nv, "y": y}, [(nv, y)]


def lanczos_plain(v, s, dinv=None):
    c1, c2 = s
    return {"v_hat_old": v["av"] - c1 * v["v_hat"] - c2 * v["v_hat_old"]}, []


def minres_wx(v, s, dinv=None, scaled=False):
    """minres.c:172-180; the new w is written over w_old"""
    r1, r2, r3, c_eta, vdiv = s
    with np.errstate(divide="ignore", invalid="ignore"):
        vv = v["v"] / vdiv if scaled else v["v"]
        nw = (vv - r3 * v["w_old"] - r2 * v["w"]) / r1
        return {"w_old": nw, "x": v["x"] + c_eta * nw}, []


def minres_wx_vnext(v, s, dinv=None):
    """the same with the scalars the kernel has without a device state (all zero, the next beta 1), and v = ynext / beta"""
    out, _ = minres_wx(v, [0.0, 0.0, 0.0, 0.0, 1.0])
    out["v"] = v["ynext"] / 1.0
    return out, []


def _p(vecs, scal, always, with_pre=(), dinv=False, pre=False, nsums=0, kry=0):
    return {"vecs": vecs.split(), "scal": scal.split(), "always": set(always.split()), "with_pre": set(with_pre),
            "dinv": dinv, "pre": pre, "nsums": nsums, "kry": kry}


# in the order of the header's enum.  pre: takes a preconditioner; kry: how many scalars it reads from a device state
PASSES = {
    "lin2": _p("x y z", "a b", "x y z"),
    "scal": _p("x", "a", "x"),
    "bicg_p": _p("r v p phat", "beta omega", "r v p", ["phat"], dinv=True, pre=True, kry=2),
    "bicg_s": _p("r v s shat", "alpha", "r v s", ["shat"], dinv=True, pre=True, kry=1),
    "bicg_xr": _p("x phat shat s t r rhat", "alpha omega", "x phat shat s t r rhat", nsums=2, kry=2),
    "cgs_q": _p("u v x q tmp2", "alpha", "u v x q tmp2", dinv=True, pre=True, kry=1),
    "cgs_r": _p("r t r0", "alpha", "r t r0", nsums=2, kry=1),
    "cgs_p": _p("r q p u kp", "beta", "r q p u", ["kp"], dinv=True, pre=True, kry=1),
    "qmrs_kv": _p("v1 wrk1", "", "v1", ["wrk1"], dinv=True, pre=True, nsums=1),
    "qmrs_pg": _p("v1 wrk1 p g", "cc", "v1 wrk1 p g", kry=1),
    "qmrs_v": _p("t v1", "beta", "t v1", nsums=1, kry=1),
    "qmrs_dx": _p("p d x v1 wrk1", "eta cc rho1inv", "p d x v1", ["wrk1"], dinv=True, pre=True, nsums=1, kry=3),
    "axpy_dot": _p("x y z", "a", "x y z", nsums=1),              # (z only when it is given)
    "axpy_dot_chain": _p("prev h_out x y z", "np_prev", "x y z", nsums=1),  # prev and h_out: scalar accesses
    "jacobi_sweep": _p("x temp y", "", "x temp y", dinv="always"),
    "dinv": _p("diag dinv", "omega", "diag dinv", nsums=1),
    "scale_div": _p("y v", "beta", "y v"),
    "lanczos": _p("av v_hat v_hat_old y", "c1 c2", "av v_hat v_hat_old", ["y"], dinv=True, pre=True, nsums=1),
    "lanczos_plain": _p("av v_hat v_hat_old", "c1 c2", "av v_hat v_hat_old"),
    "minres_wx": _p("v w w_old x", "r1 r2 r3 c_eta vdiv", "v w w_old x"),
    "minres_wx_vnext": _p("v ynext w w_old x", "", "v ynext w w_old x"),
}
FUNCS = {name: globals()[name] for name in PASSES}
KDINV = "K:dinv"


def takes_v2(name, n, misaligned, form):
    """whether the 16-byte form of `name` may run: n even and every operand the form dereferences 16-byte aligned.
    misaligned: names of the operands that sit 8 bytes off (KDINV: the preconditioner's array, which is not the vector
    `dinv` of the pass of that name); form: 'none', 'array' or 'constant'"""
    P = PASSES[name]
    reads = set(P["always"])
    if form != "none":
        reads |= P["with_pre"]
    if P["dinv"] == "always" or (P["dinv"] and form == "array"):
        reads.add(KDINV)
    return n % 2 == 0 and not (reads & set(misaligned))
