"""pysparse_amd.eigen.jdsym -- drop-in for pysparse.eigen.jdsym (jdsymmodule.c:128-315 over jdsym.c:207-621).

`jdsym(A, M, K, kmax, tau, jdtol, itmax, linsolver, ...)` runs psp_jdsym of libpysparse_hip.so: the search space, the
converged vectors and the correction equation live on the device; this module only turns Python objects into operators
(native objects through their `_psp_op` capsule, anything else with `shape` + `matvec` / `precon` through a host
callback), validates the arguments and shapes the results.  ctypes releases the GIL for the duration of the solve; the
callbacks take it back.
"""
import ctypes as C

import numpy as np

from .. import _capi
from ..itsolvers import krylov
from ._operands import _Operator, _order, _raise

__all__ = ["jdsym"]

_NATIVE = {"pcg": _capi.LIN_PCG, "minres": _capi.LIN_MINRES, "cgs": _capi.LIN_CGS, "bicgstab": _capi.LIN_BICGSTAB,
           "qmrs": _capi.LIN_QMRS, "gmres": _capi.LIN_GMRES}


def _native_solver(linsolver):
    for name, code in _NATIVE.items():
        if linsolver is getattr(krylov, name, None):
            return code
    return None


class _CorrEq(object):
    """what a foreign linear solver is handed as operator and preconditioner: the correction equation with `shape`,
    `matvec(x, y)` and `precon(x, y)` on NumPy arrays (the CorrEqSystem object of correq.c)"""

    def __init__(self, ce_a, ce_k, n):
        self._a, self._k, self.shape = ce_a, ce_k, (n, n)

    def _apply(self, op, x, y):
        n = self.shape[0]
        xx = np.ascontiguousarray(x, dtype=np.float64)
        if xx.shape != (n,) or np.shape(y) != (n,):
            raise ValueError("vector arguments of the correction equation must have %d entries" % n)
        yy = np.empty(n)
        rc = _capi.lib().psp_op_apply_host(op, xx.ctypes.data, yy.ctypes.data)
        if rc != 0:
            _raise(rc)
        y[...] = yy

    def matvec(self, x, y):
        self._apply(self._a, x, y)

    def precon(self, x, y):
        self._apply(self._k, x, y)


def jdsym(A, M, K, kmax, tau, jdtol, itmax, linsolver, jmax=25, jmin=10, blksize=1, blkwise=0, V0=None, optype=2,
          linitmax=200, eps_tr=1e-3, toldecay=1.5, clvl=0, strategy=0, projector=None):
    """kconv, lmbd, Q, it, it_inner = jdsym(A, M, K, kmax, tau, jdtol, itmax, linsolver, ...)

    Jacobi-Davidson for the kmax eigenpairs of A x = lambda M x closest to tau (A, M symmetric; M = None: the identity;
    K = None or a preconditioner for A - tau M).  Returns the number of converged pairs, their eigenvalues in order of
    convergence, the eigenvectors as a C-ordered (n, kconv) array, and the outer / inner iteration counts.

    linsolver: krylov.pcg / minres / cgs / bicgstab / qmrs / gmres of this package run their device loops on the
    correction equation; any other callable is called as linsolver(correq, b, x, tol, maxit, correq) with NumPy vectors
    and must return (info, iter, relres).  projector: an object with project(x) (in place) or a callable x -> None.

    Deviations from the reference: every condition its C code asserts (jdsym.c:133-145) raises ValueError here before
    any device call; jmax is clamped to n and jmin to jmax - 1; random start vectors are uniform (0, 1) from a
    splitmix64 hash of (fixed seed, index) generated on the device, not LAPACK's dlarnv, so iteration counts differ
    from the reference's where V0 leaves columns to fill (results are the same from run to run); a correction vector
    that comes back zero or not finite is replaced by such a pseudo-random vector (the reference divides by zero
    there); krylov.gmres as inner solver runs with the krylov module's default dim = 20; parity with the reference is
    mathematical -- eigenpairs, not iterates."""
    n = _order(A, "matrix")
    sizes = [n]
    if M is not None:
        sizes.append(_order(M, "mass matrix"))
    if K is not None:
        sizes.append(_order(K, "preconditioner"))
    if projector is not None and hasattr(projector, "shape"):
        sizes.append(_order(projector, "projector"))
    if any(s != n for s in sizes):
        raise ValueError("matrix, preconditioner or projector shapes differ")
    kmax, itmax, jmax, jmin, blksize, blkwise = int(kmax), int(itmax), int(jmax), int(jmin), int(blksize), int(blkwise)
    optype, linitmax, clvl, strategy = int(optype), int(linitmax), int(clvl), int(strategy)
    tau, jdtol, eps_tr, toldecay = float(tau), float(jdtol), float(eps_tr), float(toldecay)
    if n <= 0:
        raise ValueError("invalid matrix shape")
    if not 0.0 < jdtol:
        raise ValueError("jdtol must be positive")
    if not 0 < kmax <= n:
        raise ValueError("kmax must lie in 1 .. n")
    if not 0 < jmin < jmax:
        raise ValueError("need 0 < jmin < jmax")
    jmax_c = min(jmax, n)
    jmin_c = min(jmin, jmax_c - 1)
    if jmax_c > 128:
        raise ValueError("jmax beyond 128")
    if itmax < 0 or linitmax < 0:
        raise ValueError("itmax and linitmax must not be negative")
    if not 0 < blksize <= kmax:
        raise ValueError("blksize must lie in 1 .. kmax")
    if blksize > jmin_c:
        raise ValueError("blksize must not exceed jmin")
    if blksize > jmax_c - jmin_c:
        raise ValueError("blksize must not exceed jmax - jmin")
    if blkwise not in (0, 1):
        raise ValueError("blkwise must be 0 or 1")
    if optype not in (1, 2):
        raise ValueError("optype must be 1 (unsymmetric) or 2 (symmetric)")
    if not 0.0 <= eps_tr:
        raise ValueError("eps_tr must not be negative")
    if not 1.0 < toldecay:
        raise ValueError("toldecay must exceed 1")
    if strategy not in (0, 1):
        raise ValueError("strategy must be 0 or 1")
    if not callable(linsolver):
        raise TypeError("linsolver must be callable")
    v0 = None
    if V0 is not None:
        if not (isinstance(V0, np.ndarray) and V0.ndim in (1, 2) and V0.dtype == np.float64 and V0.shape[0] == n
                and (V0.ndim == 1 or V0.shape[1] >= 1)):
            raise ValueError("V0 is not of correct type or shape")
        v0 = V0 if all(s % 8 == 0 for s in V0.strides) else np.ascontiguousarray(V0)

    L = _capi.lib()
    ops, state = [], {"error": None}
    try:
        opA = _Operator(A, n, False)
        ops.append(opA)
        opM = opK = None
        if M is not None:
            opM = _Operator(M, n, False)
            ops.append(opM)
        if K is not None:
            opK = _Operator(K, n, True)
            ops.append(opK)

        p = _capi.JdsymParams()
        p.kmax, p.jmax, p.jmin, p.itmax, p.blksize, p.blkwise = kmax, jmax, jmin, itmax, blksize, blkwise
        p.optype, p.linitmax, p.strategy, p.clvl = optype, linitmax, strategy, clvl
        p.tau, p.jdtol, p.eps_tr, p.toldecay = tau, jdtol, eps_tr, toldecay
        native = _native_solver(linsolver)
        if native is not None:
            p.linsolver = native
        else:
            def solve(ctx, ce_a, ce_k, nn, bp, xp, tol, maxit, info_p, iter_p, relres_p):
                try:
                    ce = _CorrEq(ce_a, ce_k, nn)
                    res = linsolver(ce, np.ctypeslib.as_array(bp, (nn,)), np.ctypeslib.as_array(xp, (nn,)), tol, maxit, ce)
                    info_p[0], iter_p[0], relres_p[0] = int(res[0]), int(res[1]), float(res[2])
                    return 0
                except BaseException as e:  # noqa: B902
                    state["error"] = e
                    return 1
            p.linsolver = _capi.LIN_CALLBACK
            p.linsolve = _capi.LINSOLVE_FN(solve)
        if projector is not None:
            project = projector.project if hasattr(projector, "project") else projector

            def proj(ctx, nn, xp, yp):
                try:
                    y = np.ctypeslib.as_array(yp, (nn,))
                    y[:] = np.ctypeslib.as_array(xp, (nn,))
                    project(y)
                    return 0
                except BaseException as e:  # noqa: B902
                    state["error"] = e
                    return 1
            p.projector = _capi.HOST_APPLY_FN(proj)
        if v0 is not None:
            p.V0_host = v0.ctypes.data
            p.v0_cols = 1 if v0.ndim == 1 else v0.shape[1]
            p.v0_row_stride = v0.strides[0] // 8
            p.v0_col_stride = 0 if v0.ndim == 1 else v0.strides[1] // 8

        qbuf = np.zeros((kmax, n))  # column-major n x kmax
        lam = np.zeros(kmax)
        kconv, it, it_inner = C.c_int(0), C.c_int(0), C.c_int(0)
        rc = L.psp_jdsym(opA.ptr, opM.ptr if opM else None, opK.ptr if opK else None, n, C.byref(p), C.byref(kconv),
                         lam.ctypes.data, qbuf.ctypes.data, C.byref(it), C.byref(it_inner))
        pending = state["error"] or next((o.error for o in ops if o.error is not None), None)
        if pending is not None:
            raise pending
        if rc != 0:
            _raise(rc)
    finally:
        for o in ops:
            o.close()
    k = kconv.value
    return k, lam[:k].copy(), np.ascontiguousarray(qbuf[:k].T), it.value, it_inner.value
