"""CPU: the NumPy statements of the fused vector passes (tests/vec_passes_ref.py) are the reference's arithmetic.

tests/test_gpu_vec_passes.py compares every kernel of psp_vec.hip with those statements; what keeps that from being a
comparison of the kernels with a transcription of themselves is this file: the statements, composed into the loops of
cgs.c, bicgstab.c and qmrs.c with the scalar steps in plain Python, reproduce the oracle's solves -- info, iteration count
and the iterate to 1e-12 max|x| after ten iterations, the bar of test_gpu_solvers._check_odd_solve -- on the systems of
test_gpu_solvers._odd_systems, without a preconditioner and with Jacobi; and ten steps of the Gram-Schmidt chain of
axpy_dot reproduce modified Gram-Schmidt written out in NumPy."""
import math

import numpy as np
import pytest

import vec_passes_ref as R
from test_gpu_solvers import _odd_systems

RTOL_X = 1e-12


def _dot(pair):
    return float(np.dot(pair[0], pair[1]))


def _mv(A, x):
    y = np.empty(A.shape[0])
    A.matvec(np.ascontiguousarray(x), y)
    return y


def cgs(A, b, x, tol, maxit, dinv):
    """cgs.c:13-111 over cgs_q / cgs_r / cgs_p -> info, iter, x"""
    tmp = _mv(A, x)
    r0 = 1.0 * b + (-1.0) * tmp
    r, u, p = r0.copy(), r0.copy(), r0.copy()
    q = tmp2 = None
    rho, bnrm_sq = float(np.dot(r0, r0)), float(np.dot(b, b))
    if rho < bnrm_sq * (tol * tol):
        return 0, 0, x
    kp = p if dinv is None else p * dinv
    it = 0
    while it < maxit:
        v = _mv(A, kp)
        alpha = rho / float(np.dot(v, r0))
        out, _ = R.cgs_q({"u": u, "v": v, "x": x, "q": q, "tmp2": tmp2}, [alpha], dinv)
        q, tmp2, x = out["q"], out["tmp2"], out["x"]
        out, sums = R.cgs_r({"r": r, "t": _mv(A, tmp2), "r0": r0}, [alpha])
        r = out["r"]
        if _dot(sums[0]) < bnrm_sq * (tol * tol):
            return 0, it, x
        rho_new = _dot(sums[1])
        beta = rho_new / rho
        rho = rho_new
        out, _ = R.cgs_p({"r": r, "q": q, "p": p, "u": u, "kp": kp}, [beta], dinv)
        u, p = out["u"], out["p"]
        kp = out.get("kp", p)
        it += 1
    return -1, it, x


def bicgstab(A, b, x, tol, maxit, dinv):
    """bicgstab.c:203-298 over bicg_p / bicg_s / bicg_xr -> info, iter, x"""
    r = _mv(A, x)
    r = 1.0 * b + (-1.0) * r
    res0 = math.sqrt(float(np.dot(r, r)))
    rhat = r.copy()
    p = v = None
    alpha = omega = rho2 = 0.0
    it = 0
    while True:
        it += 1
        rho1 = float(np.dot(rhat, r))
        if rho1 == 0.0:
            return -6, it, x
        beta = 0.0 if it == 1 else (rho1 / rho2) * (alpha / omega)
        out, _ = R.bicg_p({"r": r, "v": v, "p": p}, [beta, omega], dinv, first=it == 1)
        p = out["p"]
        phat = out.get("phat", p)
        v = _mv(A, phat)
        alpha = rho1 / float(np.dot(rhat, v))
        out, _ = R.bicg_s({"r": r, "v": v}, [alpha], dinv)
        s = out["s"]
        shat = out.get("shat", s)
        t = _mv(A, shat)
        omega = float(np.dot(t, s)) / float(np.dot(t, t))
        out, sums = R.bicg_xr({"x": x, "phat": phat, "shat": shat, "s": s, "t": t, "rhat": rhat}, [alpha, omega])
        x, r = out["x"], out["r"]
        res = math.sqrt(_dot(sums[0]))
        if omega == 0.0:
            return -6, it, x
        rho2 = rho1
        if not (res / res0 > tol and it < maxit):
            break
    return (-1 if res / res0 >= tol else 0), it, x


def qmrs(A, b, x, tol, maxit, dinv):
    """qmrs.c:68-153 over qmrs_kv / qmrs_pg / qmrs_v / qmrs_dx -> info, iter, x"""
    n = len(b)
    rho0 = math.sqrt(float(np.dot(b, b)))
    v1 = b / rho0
    p, g, d, x = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    tau, c0, eps0, xi1, theta0, eta0, res_init, err = rho0, 1.0, 1.0, 1.0, 0.0, -1.0, rho0, 1.0
    it = 0
    out, sums = R.qmrs_kv({"v1": v1}, [], dinv)
    wrk1 = out.get("wrk1", v1)
    delta = _dot(sums[0])
    while err > tol and it < maxit:
        it += 1
        if eps0 == 0.0:
            return -6, it, x
        if delta == 0.0:
            return -2, it, x
        cc = xi1 * (delta / eps0)
        out, _ = R.qmrs_pg({"v1": v1, "wrk1": wrk1, "p": p, "g": g}, [cc])
        p, g = out["p"], out["g"]
        t = _mv(A, g)
        eps0 = float(np.dot(g, t))
        beta = eps0 / delta
        out, sums = R.qmrs_v({"t": t, "v1": v1}, [beta])
        v1 = out["v1"]
        rho1 = math.sqrt(_dot(sums[0]))
        xi1 = rho1
        if c0 * abs(beta) == 0.0:
            return -6, it, x
        theta = rho1 / (c0 * abs(beta))
        c1 = 1.0 / math.sqrt(theta * theta + 1.0)
        if beta * (c0 * c0) == 0.0:
            return -6, it, x
        eta0 = -eta0 * rho0 * (c1 * c1) / (beta * (c0 * c0))
        tau = tau * theta * c1
        if rho1 == 0.0:
            return -6, it, x
        d1 = theta0 * c1
        out, sums = R.qmrs_dx({"p": p, "d": d, "x": x, "v1": v1}, [eta0, d1 * d1, 1.0 / rho1], dinv)
        d, x, v1 = out["d"], out["x"], out["v1"]
        wrk1 = out.get("wrk1", v1)
        delta = _dot(sums[0])  # K v1 . v1 of the next iteration
        if xi1 == 0.0:
            return -6, it, x
        rho0, err, c0, theta0 = rho1, tau / res_init, c1, theta
    if dinv is not None:
        x = x * dinv
    return (0 if err < tol else -1), it, x


@pytest.mark.parametrize("jacobi", [False, True])
@pytest.mark.parametrize("system", ["constant", "variable"])
@pytest.mark.parametrize("solver", [cgs, bicgstab, qmrs])
def test_reference_passes_compose_into_the_oracle_solves(oracle, solver, system, jacobi):
    A = _odd_systems(oracle)[system]
    n = A.shape[0]
    b = np.random.default_rng(11).standard_normal(n)
    dinv = oracle.jacobi_dinv(A.diagonal()) if jacobi else None
    xo = np.zeros(n)
    with np.errstate(all="ignore"):
        info, it, _, _ = oracle.solve(solver.__name__, A, b, xo, 0.0, 10, ("jacobi", dinv, 1) if jacobi else None, dim=20)
    got_info, got_it, x = solver(A, b, np.zeros(n), 0.0, 10, dinv)
    assert (got_info, got_it) == (info, it)
    assert it == 10 and np.abs(xo).max() > 0.0
    assert np.abs(x - xo).max() <= RTOL_X * np.abs(xo).max(), np.abs(x - xo).max() / np.abs(xo).max()


def test_axpy_dot_chain_is_modified_gram_schmidt():
    """gmres.c:141-148: ten steps h_k = w . V_k; w -= h_k V_k and the norm of what is left, as the chain of axpy_dot forms
    them (the dot of step k + 1 rides on the axpy of step k) against the loop written out"""
    n, m = 1023, 10
    rng = np.random.default_rng(5)
    V = np.linalg.qr(rng.standard_normal((n, m)))[0].T.copy()
    w0 = rng.standard_normal(n)
    # written out
    w, h_ref = w0.copy(), []
    for k in range(m):
        h_ref.append(float(np.dot(w, V[k])))
        w = w - h_ref[-1] * V[k]
    nrm2_ref = float(np.dot(w, w))
    # the chain
    y, h = w0.copy(), [float(np.dot(w0, V[0]))]
    for k in range(m):
        out, sums = R.axpy_dot({"x": V[k], "y": y, "z": V[k + 1] if k + 1 < m else None}, [-h[k]])
        y = out["y"]
        h.append(_dot(sums[0]))
    scale = np.abs(h_ref).max()
    assert np.abs(np.array(h[:m]) - h_ref).max() <= RTOL_X * scale
    assert abs(h[m] - nrm2_ref) <= RTOL_X * nrm2_ref
    assert np.abs(y - w).max() <= RTOL_X * np.abs(w).max()
    # and the form that takes its coefficient from the sum the step before left
    out, _ = R.axpy_dot_chain({"x": V[0], "y": w0, "z": V[1]}, [1.0], h=h[0])
    first, _ = R.axpy_dot({"x": V[0], "y": w0, "z": V[1]}, [-h[0]])
    assert np.array_equal(out["y"], first["y"])


def test_table_names_every_pass_of_the_entry_point():
    from pysparse_amd import _capi
    assert list(R.PASSES) == list(_capi.VEC_PASSES)
    for name, P in R.PASSES.items():
        assert P["always"] <= set(P["vecs"]) and P["with_pre"] <= set(P["vecs"]) and not (P["always"] & P["with_pre"])
        assert bool(P["with_pre"]) <= P["pre"] and (P["dinv"] is True) == P["pre"]
        assert P["kry"] in (0, len(P["scal"]))
    assert sum(1 for P in R.PASSES.values() if P["kry"]) == 9
