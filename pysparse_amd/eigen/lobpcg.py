"""pysparse_amd.eigen.lobpcg -- the block eigensolver for the smallest eigenpairs of A x = lambda M x (no counterpart in
the reference, whose only eigensolver is jdsym).

`lobpcg(A, M, K, k, tol, itmax, X0=None)` runs psp_lobpcg of libpysparse_hip.so: the block of eigenvector
approximations, the search directions and their images under A and M live on the device, the preconditioner is applied
to the whole block of residuals at once (one block V-cycle for precon.multigrid).  Operands are taken as jdsym takes
them: native objects through their `_psp_op` capsule, anything else with `shape` + `matvec` / `precon` through a host
callback.  ctypes releases the GIL for the duration of the solve; the callbacks take it back.
"""
import ctypes as C

import numpy as np

from .. import _capi
from ._operands import _Operator, _order, _raise

__all__ = ["lobpcg"]

KMAX = 32


def lobpcg(A, M, K, k, tol, itmax, X0=None):
    """lmbd, Q, res, it = lobpcg(A, M, K, k, tol, itmax, X0=None)

    LOBPCG for the k smallest eigenpairs of A x = lambda M x: A symmetric, M symmetric positive definite (None: the
    identity), K a symmetric positive definite preconditioner for A (None: none).  1 <= k <= 32 and 3 k <= n.
    X0: a float64 array (n,) or (n, j), j <= k, of start vectors; the other columns are pseudo-random (the generator of
    jdsym: the same from run to run).  A column whose residual ||A x - theta M x||_2 is at most tol (x M-normalised) is
    soft-locked; when every column passes, the residuals are recomputed from explicit products before the call returns.

    Returns the eigenvalue approximations in ascending order, the M-orthonormal vectors as a C-ordered (n, k) array,
    the explicit residual norms and the number of iterations.  itmax reached is not an error: compare res with tol.
    Every argument check raises ValueError / TypeError before any device call."""
    n = _order(A, "matrix")
    sizes = [n]
    if M is not None:
        sizes.append(_order(M, "mass matrix"))
    if K is not None:
        sizes.append(_order(K, "preconditioner"))
    if any(s != n for s in sizes):
        raise ValueError("matrix, mass matrix or preconditioner shapes differ")
    k, itmax, tol = int(k), int(itmax), float(tol)
    if n <= 0:
        raise ValueError("invalid matrix shape")
    if not 1 <= k <= KMAX:
        raise ValueError("k must lie in 1 .. %d" % KMAX)
    if 3 * k > n:
        raise ValueError("3 k must not exceed n")
    if not 0.0 < tol:
        raise ValueError("tol must be positive")
    if itmax < 0:
        raise ValueError("itmax must not be negative")
    x0, x0_cols = None, 0
    if X0 is not None:
        if not (isinstance(X0, np.ndarray) and X0.ndim in (1, 2) and X0.dtype == np.float64 and X0.shape[0] == n
                and (X0.ndim == 1 or 1 <= X0.shape[1] <= k)):
            raise ValueError("X0 is not of correct type or shape")
        x0 = np.asfortranarray(X0.reshape(n, -1))  # column-major, leading dimension n
        x0_cols = x0.shape[1]

    L = _capi.lib()
    ops = []
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
        qbuf = np.zeros((k, n))  # column-major n x k
        lam, res = np.zeros(k), np.zeros(k)
        kconv, it = C.c_int(0), C.c_int(0)
        rc = L.psp_lobpcg(opA.ptr, opM.ptr if opM else None, opK.ptr if opK else None, n, k, tol, itmax,
                          x0.ctypes.data if x0 is not None else None, x0_cols, n, lam.ctypes.data, qbuf.ctypes.data, n,
                          res.ctypes.data, C.byref(kconv), C.byref(it))
        pending = next((o.error for o in ops if o.error is not None), None)
        if pending is not None:
            raise pending
        if rc != 0:
            _raise(rc)
    finally:
        for o in ops:
            o.close()
    return lam, np.ascontiguousarray(qbuf.T), res, it.value
