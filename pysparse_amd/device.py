"""Python handles over the C ABI (include/pysparse_hip.h) for NumPy callers.

This is the thin layer bench.py, the GPU parity tests and the multi-GPU driver use; it
mirrors the reference's operator protocol (objects with `shape` + `matvec(x, y)` /
`precon(x, y)`; `info, iter, relres = pcg(A, b, x, tol, maxit, K)`), see
doc/pysparse/source/itsolvers.rst:26-76 and precon.rst:15-24 of the reference.
All arithmetic happens in libpysparse_hip.so on the GPU; nothing here computes.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import check, lib


def _f64(a, n, what):
    if not isinstance(a, np.ndarray) or a.ndim != 1 or a.dtype != np.float64 or a.shape[0] != n:
        raise ValueError("%s must be a 1-dimensional double array of appropriate size." % what)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _block(a, rows, what, k=None, writable=False):
    """(array, leading dimension) of a 2-D float64 block with `rows` rows for the column-major C ABI.  Any strides are
    accepted: a block whose columns are contiguous (Fortran order, or a column slice of one) is passed as it is, anything
    else through a column-major copy (the second value of the returned pair tells the caller to copy back)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a 2-dimensional double array" % what)
    if a.ndim != 2 or a.dtype != np.float64 or a.shape[0] != rows or a.shape[1] < 1 or (k is not None and a.shape[1] != k):
        raise ValueError("%s must be a 2-dimensional double array of appropriate size." % what)
    if writable and not a.flags.writeable:
        raise ValueError("%s is read-only" % what)
    es = a.itemsize
    direct = (a.strides[0] == es or rows == 1) and (a.shape[1] == 1 or (a.strides[1] % es == 0 and a.strides[1] // es >= rows))
    if direct and rows >= 1:
        ld = a.strides[1] // es if a.shape[1] > 1 else max(rows, 1)
        return a, ld, False
    return np.asfortranarray(a), max(rows, 1), True


def _matmat(fn, h, shape, X, Y):
    nrows, ncols = shape
    xb, ldx, _ = _block(X, ncols, "arg 1")
    yb, ldy, copy_back = _block(Y, nrows, "arg 2", k=X.shape[1], writable=True)
    if copy_back:
        yb = np.empty((nrows, X.shape[1]), dtype=np.float64, order="F")
    check(fn(h, int(X.shape[1]), _ptr(xb), ldx, _ptr(yb), ldy))
    if copy_back:
        Y[...] = yb


PSP_MG_GALERKIN, PSP_MG_SINGLE, PSP_MG_BOX, PSP_MG_INTERP = 1, 2, 8, 16  # psp_mg_create_*_ex flags (pysparse_hip.h)


class DeviceBuffer:
    """n doubles (or raw bytes) of HBM."""

    def __init__(self, n, dtype=np.float64):
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.nbytes = self.n * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().psp_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(a.size, a.dtype)
        b.upload(a)
        return b

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size == self.n
        check(lib().psp_memcpy_h2d(self.ptr, _ptr(a), self.nbytes))

    def download(self):
        out = np.empty(self.n, dtype=self.dtype)
        check(lib().psp_memcpy_d2h(_ptr(out), self.ptr, self.nbytes))
        return out

    def zero(self):
        check(lib().psp_memset(self.ptr, 0, self.nbytes))

    def free(self):
        if getattr(self, "ptr", None):
            lib().psp_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCSR:
    """csr_mat on the GPU (csr_mat.h:6-13): shape, nnz, matvec, matvec_transp."""

    def __init__(self, handle):
        self._h = handle
        nr, nc, nz = C.c_int(), C.c_int(), C.c_int()
        check(lib().psp_csr_shape(handle, C.byref(nr), C.byref(nc), C.byref(nz)))
        self.shape = (nr.value, nc.value)
        self.nnz = nz.value if nz.value >= 0 else int(lib().psp_csr_nnz64(handle))  # > 2^31: the 64-bit count

    @classmethod
    def from_arrays64(cls, shape, ind, col, val):
        """CSR triple with 64-bit row offsets (nnz may exceed the reference's C int, csr_mat.h:6-13)"""
        ind = np.ascontiguousarray(ind, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        if ind.shape[0] != shape[0] + 1 or col.shape[0] != val.shape[0]:
            raise ValueError("inconsistent CSR arrays")
        h = C.c_void_p()
        check(lib().psp_csr_create64(shape[0], shape[1], val.shape[0], _ptr(ind), _ptr(col), _ptr(val), C.byref(h)))
        return cls(h)

    @classmethod
    def random_banded(cls, nrows, ncols, m, stride, seed=0):
        """synthetic general CSR generated on the device (nrows*m may exceed 2^31), psp_csr_random_banded"""
        h = C.c_void_p()
        check(lib().psp_csr_random_banded(nrows, ncols, m, stride, seed, C.byref(h)))
        return cls(h)

    def download_rows(self, row_lo, row_hi):
        """(ind64 relative to row_lo, col, val) of rows [row_lo, row_hi)"""
        ind = np.empty(row_hi - row_lo + 1, dtype=np.int64)
        check(lib().psp_csr_download_rows(self._h, row_lo, row_hi, _ptr(ind), None, None))
        col = np.empty(int(ind[-1]), dtype=np.int32)
        val = np.empty(int(ind[-1]), dtype=np.float64)
        check(lib().psp_csr_download_rows(self._h, row_lo, row_hi, _ptr(ind), _ptr(col), _ptr(val)))
        return ind, col, val

    @classmethod
    def from_arrays(cls, shape, ind, col, val):
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        if ind.shape[0] != shape[0] + 1 or col.shape[0] != val.shape[0]:
            raise ValueError("inconsistent CSR arrays")
        h = C.c_void_p()
        check(lib().psp_csr_create(shape[0], shape[1], val.shape[0], _ptr(ind), _ptr(col), _ptr(val),
                                   C.byref(h)))
        return cls(h)

    @classmethod
    def poisson(cls, nx, ny, nz=0):
        h = C.c_void_p()
        check(lib().psp_csr_poisson(nx, ny, nz, C.byref(h)))
        return cls(h)

    @classmethod
    def poisson_multi(cls, nx, ny, nz=0, devices=(0,)):
        """the Poisson operator as row slabs on a LIST of devices, one process (psp_csr_poisson_multi): matvec,
        DeviceJacobi(A), pcg and minres work on it; a device may be listed more than once"""
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        check(lib().psp_csr_poisson_multi(nx, ny, nz, _ptr(dv), len(dv), C.byref(h)))
        A = cls(h)
        A.nnz = int(lib().psp_csr_nnz64(h))
        return A

    @classmethod
    def from_arrays_multi(cls, shape, ind, col, val, devices=(0,)):
        """any square CSR matrix as row blocks on a list of devices (psp_csr_create_multi)"""
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        if ind.shape[0] != shape[0] + 1 or col.shape[0] != val.shape[0]:
            raise ValueError("inconsistent CSR arrays")
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        check(lib().psp_csr_create_multi(shape[0], shape[1], val.shape[0], _ptr(ind), _ptr(col), _ptr(val),
                                         _ptr(dv), len(dv), C.byref(h)))
        return cls(h)

    def multi_info(self):
        """(ranks, distinct devices, reductions through RCCL) -- (0, 0, False) for a single-device matrix"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().psp_csr_multi_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, bool(c.value)

    @classmethod
    def poisson_big(cls, nx, ny, nz=0):
        """the Poisson operator in the index-free w4 layout only (nnz may exceed 32 bits: 1024^3)"""
        h = C.c_void_p()
        check(lib().psp_csr_poisson_big(nx, ny, nz, C.byref(h)))
        A = cls(h)
        A.nnz = int(lib().psp_csr_nnz64(h))
        return A

    @classmethod
    def poisson_big_slab(cls, nx, ny, nz, row_lo, row_hi, col_shift, ncols_local):
        """row slab of the index-free operator (per-rank nnz may exceed 32 bits: 1024^3 over 2 GPUs)"""
        h = C.c_void_p()
        check(lib().psp_csr_poisson_big_slab(nx, ny, nz, row_lo, row_hi, col_shift, ncols_local, C.byref(h)))
        A = cls(h)
        A.nnz = int(lib().psp_csr_nnz64(h))
        return A

    @classmethod
    def poisson_slab(cls, nx, ny, nz, row_lo, row_hi, col_shift, ncols_local):
        h = C.c_void_p()
        check(lib().psp_csr_poisson_slab(nx, ny, nz, row_lo, row_hi, col_shift, ncols_local, C.byref(h)))
        return cls(h)

    def matvec(self, x, y):
        _f64(x, self.shape[1], "arg 1")
        _f64(y, self.shape[0], "arg 2")
        es = x.itemsize
        check(lib().psp_csr_matvec_stride(self._h, _ptr(x), x.strides[0] // es, _ptr(y), y.strides[0] // es))

    def matmat(self, X, Y):
        """Y[:, c] = A X[:, c] for every column: X (ncols, k), Y (nrows, k), 2-D float64 with any strides.  One block
        product (psp_csr_matmat); column c has the bits of matvec on X[:, c]."""
        _matmat(lib().psp_csr_matmat, self._h, self.shape, X, Y)

    def matmat_dev(self, k, x_ptr, ldx, y_ptr, ldy):
        check(lib().psp_csr_matmat_dev(self._h, int(k), x_ptr, int(ldx), y_ptr, int(ldy)))

    def matvec_transp(self, x, y):
        _f64(x, self.shape[0], "arg 1")
        _f64(y, self.shape[1], "arg 2")
        es = x.itemsize
        check(lib().psp_csr_matvec_transp_stride(self._h, _ptr(x), x.strides[0] // es, _ptr(y),
                                                 y.strides[0] // es))

    def matvec_dev(self, x_ptr, y_ptr):
        check(lib().psp_csr_matvec_dev(self._h, x_ptr, y_ptr))

    def download(self):
        ind = np.empty(self.shape[0] + 1, dtype=np.int32)
        col = np.empty(self.nnz, dtype=np.int32)
        val = np.empty(self.nnz, dtype=np.float64)
        check(lib().psp_csr_download(self._h, _ptr(ind), _ptr(col), _ptr(val)))
        return ind, col, val

    def diagonal(self):
        d = np.empty(self.shape[0])
        check(lib().psp_csr_diagonal(self._h, _ptr(d)))
        return d

    def set_variant(self, v):
        check(lib().psp_csr_set_variant(self._h, int(v)))

    def set_schedule(self, strip_rows):
        check(lib().psp_csr_set_schedule(self._h, int(strip_rows)))

    def kernel_info(self):
        """(kernel name, {nb, max_blocks, scheduled, half_band}) of the product y = A x."""
        name = C.create_string_buffer(160)
        info = (C.c_int * 4)()
        check(lib().psp_csr_kernel_info(self._h, name, 160, info))
        return name.value.decode(), {"nb": info[0], "max_blocks": info[1], "scheduled": bool(info[2]),
                                     "half_band": info[3], "setup_ms": self.setup_info()["reorder_ms"]}

    def release_arrays(self):
        """psp_csr_release_arrays: an offset-structured operator keeps its index-free tables only (no download, no
        variants afterwards): 1.65 x -> 1.0 x device memory"""
        check(lib().psp_csr_release_arrays(self._h))

    def prepare(self, expected_products):
        """psp_csr_prepare: the caller expects about this many products / solver iterations with this handle -- whatever
        pays for itself within them (the renumbered copy of an irregular numbering: from 2048 on) is built at the next
        product instead of after that many have been counted"""
        check(lib().psp_csr_prepare(self._h, int(expected_products)))

    def setup_info(self):
        v = (C.c_double * 4)()
        check(lib().psp_csr_setup_info(self._h, v))
        return {"reorder_ms": v[0], "products_counted": int(v[1]), "reorder_after": int(v[2]), "reorder_state": int(v[3])}

    def renumbering(self):
        """perm[new] = old row of the renumbered copy behind csr_spmv_w3_rcm, or None when the handle has none."""
        perm = np.empty(self.shape[0], dtype=np.int32)
        have = C.c_int()
        check(lib().psp_csr_renumbering(self._h, perm.ctypes.data, C.byref(have)))
        self.renumbered_on = {0: None, 1: "host", 2: "device"}[have.value]
        return perm if have.value else None

    @property
    def device_bytes(self):
        return lib().psp_csr_device_bytes(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_csr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSSS:
    """sss_mat on the GPU (sss_mat.h:6-14); nnz = strict-lower count + n (sss_mat.c:155)."""

    def __init__(self, handle):
        self._h = handle
        n, nz = C.c_int(), C.c_int()
        check(lib().psp_sss_shape(handle, C.byref(n), C.byref(nz)))
        self.n = n.value
        self.shape = (self.n, self.n)
        self.nnz = nz.value

    @classmethod
    def from_arrays(cls, n, ind, col, val, diag):
        ind = np.ascontiguousarray(ind, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        diag = np.ascontiguousarray(diag, dtype=np.float64)
        h = C.c_void_p()
        check(lib().psp_sss_create(n, val.shape[0], _ptr(ind), _ptr(col), _ptr(val), _ptr(diag), C.byref(h)))
        return cls(h)

    @classmethod
    def poisson(cls, nx, ny, nz=0):
        h = C.c_void_p()
        check(lib().psp_sss_poisson(nx, ny, nz, C.byref(h)))
        return cls(h)

    def matvec(self, x, y):
        _f64(x, self.n, "arg 1")
        _f64(y, self.n, "arg 2")
        es = x.itemsize
        check(lib().psp_sss_matvec_stride(self._h, _ptr(x), x.strides[0] // es, _ptr(y), y.strides[0] // es))

    matvec_transp = matvec  # sss_mat.c:108

    def matmat(self, X, Y):
        """Y[:, c] = A X[:, c] for every column (psp_sss_matmat): X, Y (n, k), 2-D float64 with any strides."""
        _matmat(lib().psp_sss_matmat, self._h, (self.n, self.n), X, Y)

    def matmat_dev(self, k, x_ptr, ldx, y_ptr, ldy):
        check(lib().psp_sss_matmat_dev(self._h, int(k), x_ptr, int(ldx), y_ptr, int(ldy)))

    def matvec_dev(self, x_ptr, y_ptr):
        check(lib().psp_sss_matvec_dev(self._h, x_ptr, y_ptr))

    def set_variant(self, v):
        check(lib().psp_sss_set_variant(self._h, int(v)))

    def prepare(self, expected_products):
        """psp_sss_prepare (see DeviceCSR.prepare)"""
        check(lib().psp_sss_prepare(self._h, int(expected_products)))

    def setup_info(self):
        v = (C.c_double * 4)()
        check(lib().psp_sss_setup_info(self._h, v))
        return {"reorder_ms": v[0], "products_counted": int(v[1]), "reorder_after": int(v[2]), "reorder_state": int(v[3])}

    def kernel_info(self):
        name = C.create_string_buffer(64)
        info = (C.c_int * 4)()
        check(lib().psp_sss_kernel_info(self._h, name, 64, info))
        return name.value.decode(), {"nb": info[0], "max_blocks": info[1], "scheduled": bool(info[2]),
                                     "half_band": info[3], "setup_ms": self.setup_info()["reorder_ms"]}

    def __getitem__(self, ij):
        if not (isinstance(ij, tuple) and len(ij) == 2 and all(isinstance(t, (int, np.integer)) for t in ij)):
            raise IndexError("slices not supported")
        i, j = int(ij[0]), int(ij[1])
        if i < 0:
            i += self.n
        if j < 0:
            j += self.n
        if not (0 <= i < self.n and 0 <= j < self.n):
            raise IndexError("indices out of range")
        v = C.c_double()
        check(lib().psp_sss_getitem(self._h, i, j, C.byref(v)))
        return v.value

    def download(self):
        nl = self.nnz - self.n
        ind = np.empty(self.n + 1, dtype=np.int32)
        col = np.empty(nl, dtype=np.int32)
        val = np.empty(nl, dtype=np.float64)
        diag = np.empty(self.n, dtype=np.float64)
        check(lib().psp_sss_download(self._h, _ptr(ind), _ptr(col), _ptr(val), _ptr(diag)))
        return ind, col, val, diag

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_sss_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Op:
    """psp_op_t wrapper; keeps the Python object and the ctypes callback alive."""

    def __init__(self, obj, method):
        self.obj = obj
        self.exc = None
        h = C.c_void_p()
        if isinstance(obj, DeviceCSR):
            check(lib().psp_op_from_csr(obj._h, C.byref(h)))
        elif isinstance(obj, DeviceSSS):
            check(lib().psp_op_from_sss(obj._h, C.byref(h)))
        elif isinstance(obj, DeviceJacobi):
            check(lib().psp_op_from_jacobi(obj._h, C.byref(h)))
        elif isinstance(obj, DeviceSSOR):
            check(lib().psp_op_from_ssor(obj._h, C.byref(h)))
        elif isinstance(obj, DeviceMultigrid):
            check(lib().psp_op_from_mg(obj._h, C.byref(h)))
        else:
            # duck-typed operator: shape + matvec/precon (spmatrixmodule.c:86-132, :169-248)
            shape = obj.shape
            if len(shape) != 2:
                raise ValueError("invalid matrix shape")
            if int(shape[0]) != int(shape[1]):
                raise ValueError("matrix is not square")
            n = int(shape[0])
            fn = getattr(obj, method)

            def trampoline(ctx, nn, xp, yp):
                try:
                    x = np.ctypeslib.as_array(xp, shape=(nn,))
                    y = np.ctypeslib.as_array(yp, shape=(nn,))
                    fn(x, y)
                    return 0
                except BaseException as e:  # noqa: BLE001 - re-raised by the caller
                    self.exc = e
                    return 1

            self._cb = _capi.HOST_APPLY_FN(trampoline)
            check(lib().psp_op_from_callback(n, self._cb, None, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_op_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceJacobi:
    """precon.jacobi(A, omega=1.0, steps=1) (preconmodule.c:352-412, :470-485)."""

    def __init__(self, A, omega=1.0, steps=1):
        h = C.c_void_p()
        self._A = A
        self._aop = None
        if isinstance(A, DeviceCSR):
            check(self._map(lib().psp_jacobi_create_csr(A._h, omega, steps, C.byref(h))))
            n = A.shape[0]
        elif isinstance(A, DeviceSSS):
            check(self._map(lib().psp_jacobi_create_sss(A._h, omega, steps, C.byref(h))))
            n = A.n
        else:
            shape = A.shape
            if int(shape[0]) != int(shape[1]):
                raise ValueError("matrix is not square")
            n = int(shape[0])
            diag = np.array([float(A[i, i]) for i in range(n)])  # preconmodule.c:389-392
            if steps > 1:
                self._aop = _Op(A, "matvec")
            check(self._map(lib().psp_jacobi_create_diag(n, _ptr(diag), omega, steps,
                                                         self._aop._h if self._aop else None, C.byref(h))))
        self._h = h
        self.shape = (n, n)

    @staticmethod
    def _map(rc):
        if rc == -4:  # PSP_ESINGULAR -> the reference's ValueError (preconmodule.c:396)
            raise ValueError("diagonal element close to zero")
        return rc

    def precon(self, x, y):
        n = self.shape[0]
        for k, a in ((1, x), (2, y)):
            if (not isinstance(a, np.ndarray) or a.ndim != 1 or a.dtype != np.float64 or a.shape[0] != n
                    or not a.flags.c_contiguous):
                raise ValueError("arg %d must be a contiguous 1-dimensional double array of appropriate size." % k)
        check(lib().psp_jacobi_precon(self._h, _ptr(x), _ptr(y)))

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_jacobi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSSOR:
    """precon.ssor(A, omega=1.0, steps=1) on an sss_mat (preconmodule.c:414-459, :95-223)."""

    def __init__(self, A, omega=1.0, steps=1):
        if not isinstance(A, DeviceSSS):
            raise TypeError("ssor() argument 1 must be sss_mat")  # "O!" with SSSMatType, preconmodule.c:499
        h = C.c_void_p()
        check(lib().psp_ssor_create(A._h, float(omega), int(steps), C.byref(h)))
        self._A = A  # the handle borrows the matrix
        self._h = h
        self.shape = (A.n, A.n)
        lf, lb = C.c_int(), C.c_int()
        check(lib().psp_ssor_info(h, None, C.byref(lf), C.byref(lb)))
        self.levels = (lf.value, lb.value)
        rf, rb, lv, sl = C.c_int(), C.c_int(), C.c_long(), C.c_long()
        check(lib().psp_ssor_run_info(h, C.byref(rf), C.byref(rb), C.byref(lv), C.byref(sl)))
        # (runs forward, runs backward, levels covered, slots covered) of the LDS-exchange runs of narrow levels
        self.lds_runs = (rf.value, rb.value, lv.value, sl.value)
        nbr, edge = C.c_int(), C.c_int()
        check(lib().psp_ssor_brick_info(h, C.byref(nbr), C.byref(edge)))
        self.bricks = nbr.value  # 3-D grid operators with wide levels: bricks of edge^3 points, 0 otherwise

    def precon(self, x, y):
        n = self.shape[0]
        for k, a in ((1, x), (2, y)):
            if (not isinstance(a, np.ndarray) or a.ndim != 1 or a.dtype != np.float64 or a.shape[0] != n
                    or not a.flags.c_contiguous):
                raise ValueError("arg %d must be a contiguous 1-dimensional double array of appropriate size." % k)
        check(lib().psp_ssor_precon(self._h, _ptr(x), _ptr(y)))

    def precon_dev(self, x_ptr, y_ptr):
        check(lib().psp_ssor_precon_dev(self._h, x_ptr, y_ptr))

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_ssor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_einval(rc):
    """PSP_EINVAL of a constructor -> ValueError with the library's text, anything else as check() raises it"""
    if rc == -1:
        raise ValueError(lib().psp_last_error().decode())
    return check(rc)


class DeviceMultigrid:
    """precon.multigrid(A, grid, omega=0.8, steps=2, galerkin=False): a matrix-free geometric V-cycle for the
    constant-coefficient grid operators A = sum_a c_a T_a + s I (psp_mg.hip; no reference analogue).  `levels` are the
    level grids, finest first.  galerkin=True: the same cycle for any symmetric 3- / 5- / 7-point operator on the grid
    (varying coefficients) with stored level operators A_{l+1} = R A_l P.  The subclass
    DeviceMultigrid32 is the single-precision cycle of either mode."""

    _FLAGS = 0  # ORed into psp_mg_create_*_ex's flags; DeviceMultigrid32 sets PSP_MG_SINGLE

    def __init__(self, A, grid, omega=0.8, steps=2, galerkin=False):
        self._create(A, grid, omega, steps, galerkin, None)

    def _create(self, A, grid, omega, steps, galerkin, line, stencil="axis", interp="linear"):
        """every check, then the handle; line: None, or the axis of DeviceMultigridLine; stencil: 'axis', or
        DeviceMultigridBox's 'box'; interp: 'linear', or DeviceMultigridInterp's 'operator'"""
        if not isinstance(galerkin, bool):
            raise TypeError("galerkin must be a bool")
        if not isinstance(interp, str):
            raise TypeError("interp must be a str, 'linear' or 'operator'")
        if interp not in ("linear", "operator"):
            raise ValueError("interp must be 'linear' or 'operator'")
        if interp == "operator":
            if not galerkin:
                raise ValueError("interp='operator' needs galerkin=True: the weights come from stored level operators")
            if line is not None:
                raise ValueError("interp='operator' with line is not supported")
            if self._FLAGS & PSP_MG_SINGLE:
                raise ValueError("interp='operator' with precision='single' is not supported")
        if not isinstance(stencil, str):
            raise TypeError("stencil must be a str, 'axis' or 'box'")
        if stencil not in ("axis", "box"):
            raise ValueError("stencil must be 'axis' or 'box'")
        box = stencil == "box"
        if box and not galerkin:
            raise ValueError("stencil='box' needs galerkin=True: the matrix-free mode stores no level operators")
        if box and line is not None:
            raise ValueError("stencil='box' with line: the line smoother on 9- / 27-point operators is not supported")
        if line is not None and (isinstance(line, bool) or not isinstance(line, int)):
            raise TypeError("line must be None or an int, the axis of the line smoother")
        if not isinstance(A, (DeviceCSR, DeviceSSS)):
            raise TypeError("multigrid() argument 1 must be a csr_mat or sss_mat handle")
        if isinstance(grid, (str, bytes)) or not hasattr(grid, "__len__") or not hasattr(grid, "__getitem__"):
            raise TypeError("multigrid() argument 2 must be a sequence of 1 to 3 positive integers")
        if not 1 <= len(grid) <= 3:
            raise ValueError("grid must have 1 to 3 axes")
        dims = []
        for g in grid:
            if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
                raise TypeError("grid axes must be integers")
            if g < 1:
                raise ValueError("grid axes must be positive integers")
            dims.append(int(g))
        shape = A.shape if isinstance(A, DeviceCSR) else (A.n, A.n)
        if shape[0] != shape[1]:
            raise ValueError("matrix is not square")
        if int(np.prod(dims, dtype=object)) != shape[0]:
            raise ValueError("prod(grid) does not match the matrix order")
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
            raise TypeError("steps must be an integer")
        omega, steps = float(omega), int(steps)
        if not 0.0 < omega <= 1.0:
            raise ValueError("omega must satisfy 0 < omega <= 1")
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if line is not None:
            if not galerkin:
                raise ValueError("line needs galerkin=True: the line smoother works on stored level operators")
            if self._FLAGS & PSP_MG_SINGLE:
                raise ValueError("line with precision='single': the line smoother has no single-precision form")
            if len(dims) < 2:
                raise ValueError("line on a grid of one axis: there is no axis left to coarsen")
            if not 0 <= line < len(dims):
                raise ValueError("line must be one of the grid's axes, 0 .. %d" % (len(dims) - 1))
            if dims[line] < 2:
                raise ValueError("the line axis must have at least 2 points")
        h = C.c_void_p()
        g = (C.c_int * len(dims))(*dims)
        if line is not None:
            create = lib().psp_mg_create_csr_line if isinstance(A, DeviceCSR) else lib().psp_mg_create_sss_line
            _check_einval(create(A._h, len(dims), g, omega, steps, line, C.byref(h)))
        else:
            create = lib().psp_mg_create_csr_ex if isinstance(A, DeviceCSR) else lib().psp_mg_create_sss_ex
            flags = (PSP_MG_GALERKIN if galerkin else 0) | (PSP_MG_BOX if box else 0) | self._FLAGS
            if interp == "operator":
                flags |= PSP_MG_INTERP
            _check_einval(create(A._h, len(dims), g, omega, steps, flags, C.byref(h)))
        self._A = A
        self._h = h
        self.shape = (shape[0], shape[0])
        self.ndim = len(dims)
        self.levels = tuple(lv[:self.ndim] for lv in self.info()["dims"])

    @property
    def stencil(self):
        """'axis' (3- / 5- / 7-point operators) or 'box' (9- / 27-point ones, DeviceMultigridBox); read-only"""
        return self.info()["stencil"]

    def info(self):
        """levels, first level of the single-workgroup tail launch, kernel launches per application, level dimensions
        (three per level, 1 on absent axes), whether the handle stores Galerkin level operators, and the precision
        of the cycle ('double' or 'single'), and the axis of the line smoother (None without one; with one there is no
        tail launch and tail_first_level == levels), and the pattern of the accepted operators ('axis', or 'box' for
        DeviceMultigridBox)"""
        nl, tf, la, gk, bits, ax, bx = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(lib().psp_mg_stencil(self._h, C.byref(bx)))
        check(lib().psp_mg_is_galerkin(self._h, C.byref(gk)))
        check(lib().psp_mg_precision(self._h, C.byref(bits)))
        check(lib().psp_mg_line_axis(self._h, C.byref(ax)))
        check(lib().psp_mg_info(self._h, C.byref(nl), C.byref(tf), C.byref(la), None))
        d = (C.c_int * (3 * nl.value))()
        check(lib().psp_mg_info(self._h, None, None, None, d))
        return {"levels": nl.value, "tail_first_level": tf.value, "launches_per_apply": la.value,
                "dims": tuple(tuple(d[3 * l:3 * l + 3]) for l in range(nl.value)), "galerkin": bool(gk.value),
                "precision": "single" if bits.value == 32 else "double", "line": ax.value if ax.value >= 0 else None,
                "stencil": "box" if bx.value else "axis"}

    @property
    def interp(self):
        """'linear', or 'operator' for DeviceMultigridInterp's operator-dependent interpolation; read-only"""
        op = C.c_int()
        check(lib().psp_mg_interp(self._h, C.byref(op)))
        return "operator" if op.value else "linear"

    def interp_fallbacks(self, level):
        """test hook (interp='operator'): the points of `level` that took the linear weights (psp_mg_interp_fallbacks)"""
        pts = C.c_longlong()
        _check_einval(lib().psp_mg_interp_fallbacks(self._h, int(level), C.byref(pts)))
        return pts.value

    def transfer_weights(self, level):
        """test hook (interp='operator'): W[slot, point], the weights of the prolongation onto `level`; bit a of the slot
        number names the parent along axis a, 0 the lower (or only) one, 1 the upper one (psp_mg_transfer_weights)"""
        cnt = C.c_int(0)
        _check_einval(lib().psp_mg_transfer_weights(self._h, int(level), C.byref(cnt), None))
        W = np.empty((cnt.value, int(np.prod(self.info()["dims"][level]))))
        check(lib().psp_mg_transfer_weights(self._h, int(level), C.byref(cnt), _ptr(W)))
        return W

    def bytes(self):
        """{"operator", "vector"}: device bytes the handle holds at rest (psp_mg_bytes) -- the level operators with the
        coarsest inverse and the tail's table, and the level vectors; the block cycle's vectors are block_info()'s"""
        ob, vb = C.c_longlong(), C.c_longlong()
        check(lib().psp_mg_bytes(self._h, C.byref(ob), C.byref(vb)))
        return {"operator": ob.value, "vector": vb.value}

    def level_operator(self, level):
        """test hook (galerkin=True): ((d0, d1, d2) per stored array, values[array, point]) of a level's symmetric stencil,
        the diagonal first; array o holds A_l[K, K+o] at point K, 0 where that neighbour does not exist"""
        cnt = C.c_int(0)
        _check_einval(lib().psp_mg_level_operator(self._h, int(level), None, C.byref(cnt), None))
        offs = (C.c_int * (3 * cnt.value))()
        npts = int(np.prod(self.info()["dims"][level]))
        vals = np.empty((cnt.value, npts))
        check(lib().psp_mg_level_operator(self._h, int(level), offs, C.byref(cnt), _ptr(vals)))
        return tuple(tuple(offs[3 * k:3 * k + 3]) for k in range(cnt.value)), vals

    def precon(self, x, y):
        n = self.shape[0]
        for k, a in ((1, x), (2, y)):
            if (not isinstance(a, np.ndarray) or a.ndim != 1 or a.dtype != np.float64 or a.shape[0] != n
                    or not a.flags.c_contiguous):
                raise ValueError("arg %d must be a contiguous 1-dimensional double array of appropriate size." % k)
        check(lib().psp_mg_precon(self._h, _ptr(x), _ptr(y)))

    def precon_dev(self, x_ptr, y_ptr):
        check(lib().psp_mg_precon_dev(self._h, x_ptr, y_ptr))

    def precon_block(self, X, Y):
        """Y[:, c] = K X[:, c] for every column in one block cycle (psp_mg_precon_block): X, Y (n, k),
        2-D float64 with any strides.  Column c has the bits of precon on X[:, c]; the launches do not grow with k."""
        _matmat(lib().psp_mg_precon_block, self._h, self.shape, X, Y)

    def precon_block_dev(self, k, x_ptr, ldx, y_ptr, ldy):
        _check_einval(lib().psp_mg_precon_block_dev(self._h, int(k), x_ptr, int(ldx), y_ptr, int(ldy)))

    def block_reserve(self, k):
        """allocate the block cycle's level vectors for at least k columns ahead of the first call; k = 0 frees them"""
        _check_einval(lib().psp_mg_block_reserve(self._h, int(k)))

    def block_info(self):
        """{"columns", "bytes"}: what the block cycle's level vectors hold now (0, 0 before the first block call)"""
        cols, nbytes = C.c_int(), C.c_longlong()
        check(lib().psp_mg_block_info(self._h, C.byref(cols), C.byref(nbytes)))
        return {"columns": cols.value, "bytes": nbytes.value}

    def close(self):
        if getattr(self, "_h", None):
            lib().psp_mg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceMultigrid32(DeviceMultigrid):
    """precon.multigrid(..., precision='single'): DeviceMultigrid's cycle, either mode, evaluated in float32 on level
    operators rounded once from the double ones.  x and y stay float64; every method is the parent's."""

    _FLAGS = PSP_MG_SINGLE


class DeviceMultigridLine(DeviceMultigrid):
    """precon.multigrid(..., galerkin=True, line=a): the Galerkin cycle with a line smoother along axis `line`, for grids
    graded or stretched along that axis (psp_mg_create_*_line).  Axis `line` is never coarsened, the
    smoother solves the tridiagonal part of every level operator along each of its grid lines exactly.  line=None is
    DeviceMultigrid.  Every method is the parent's; info()["line"] is the axis."""

    def __init__(self, A, grid, omega=0.8, steps=2, galerkin=True, line=None):
        self._create(A, grid, omega, steps, galerkin, line)


class DeviceMultigridBox(DeviceMultigrid):
    """precon.multigrid(..., galerkin=True, stencil='box'): the Galerkin cycle for symmetric operators with the full
    pattern {-1, 0, 1}^ndim -- 9 points in 2-D, 27 in 3-D (PSP_MG_BOX).  Level 0 is stored like every lower
    level.  stencil='axis' is DeviceMultigrid; precision='single' is the float32 cycle of DeviceMultigrid32.  Every
    method is the parent's; info()["stencil"] and .stencil say which pattern the handle takes."""

    def __init__(self, A, grid, omega=0.8, steps=2, galerkin=True, stencil="box", precision="double"):
        if not isinstance(precision, str):
            raise TypeError("precision must be a str, 'double' or 'single'")
        if precision not in ("double", "single"):
            raise ValueError("precision must be 'double' or 'single'")
        self._FLAGS = PSP_MG_SINGLE if precision == "single" else 0
        self._create(A, grid, omega, steps, galerkin, None, stencil)


class DeviceMultigridInterp(DeviceMultigrid):
    """precon.multigrid(..., galerkin=True, interp='operator'): the Galerkin cycle with operator-dependent interpolation,
    the weights of every level derived from the level operator's own stencil, for coefficients that jump between regions
    (PSP_MG_INTERP).  stencil is 'axis' or 'box'; interp='linear' is DeviceMultigrid / DeviceMultigridBox.
    Double precision, no line smoother.  Every method is the parent's; .interp says which transfer the handle has."""

    def __init__(self, A, grid, omega=0.8, steps=2, galerkin=True, stencil="axis", interp="operator"):
        self._create(A, grid, omega, steps, galerkin, None, stencil, interp)


def _solve(fn, A, b, x, tol, maxit, K, hist):
    aop = _Op(A, "matvec")
    kop = _Op(K, "precon") if K is not None else None
    n = int(A.shape[0])
    # ItSolvers_pcg (itsolversmodule.c:70-88): x is updated in place only when it already is
    # a contiguous float64 array; anything else is converted, solved and discarded
    xw = x if (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous
               and x.ndim == 1) else np.ascontiguousarray(x, dtype=np.float64)
    bw = np.ascontiguousarray(b, dtype=np.float64)
    if xw.ndim != 1 or bw.ndim != 1 or xw.shape[0] != bw.shape[0] or xw.shape[0] != n:
        raise ValueError("incompatible operand shapes")
    info, it, rr = C.c_int(0), C.c_int(0), C.c_double(0.0)
    h = np.full(maxit + 2, np.nan) if hist else None
    rc = fn(aop._h, kop._h if kop else None, n, _ptr(xw), _ptr(bw), float(tol), int(maxit),
            C.byref(info), C.byref(it), C.byref(rr), _ptr(h) if hist else None)
    for op in (aop, kop):
        if op is not None and op.exc is not None:
            raise op.exc
    check(rc)
    res = (info.value, it.value, rr.value)
    return res + (h,) if hist else res


def pcg(A, b, x, tol, maxit, K=None, hist=False):
    """info, iter, relres = pcg(A, b, x, tol, maxit[, K]) -- itsolversmodule.c:32-118."""
    return _solve(lib().psp_pcg, A, b, x, tol, maxit, K, hist)


def minres(A, b, x, tol, maxit, K=None, hist=False):
    """info, iter, relres = minres(A, b, x, tol, maxit[, K]) -- itsolversmodule.c:217-305."""
    return _solve(lib().psp_minres, A, b, x, tol, maxit, K, hist)


def pcg_batch(A, B, X, tol, maxit, K=None):
    """info, iter, relres = pcg_batch(A, B, X, tol, maxit[, K]): pcg for the k columns of B at once (psp_pcg_batch), three
    arrays of length k.  B and X are (n, k) float64 blocks with any strides; X holds the initial guesses and is updated
    in place.  Column c ends exactly as pcg(A, B[:, c], X[:, c], tol, maxit, K) would.  A and K: what pcg accepts; a
    matrix on a device list raises ValueError."""
    n = int(A.shape[0])
    if not isinstance(B, np.ndarray) or not isinstance(X, np.ndarray):
        raise TypeError("B and X must be 2-dimensional double arrays")
    if B.ndim != 2 or X.ndim != 2 or B.shape != X.shape or B.shape[0] != n or B.shape[1] < 1:
        raise ValueError("incompatible operand shapes")
    if B.dtype != np.float64 or X.dtype != np.float64:
        raise ValueError("B and X must be double arrays")
    if not X.flags.writeable:
        raise ValueError("X is read-only")
    k = int(B.shape[1])
    aop = _Op(A, "matvec")
    kop = _Op(K, "precon") if K is not None else None
    bb, ldb, _ = _block(B, n, "B")
    xb, ldx, copy_back = _block(X, n, "X", k=k, writable=True)
    info = np.zeros(k, dtype=np.intc)
    it = np.zeros(k, dtype=np.intc)
    rr = np.zeros(k, dtype=np.float64)
    rc = lib().psp_pcg_batch(aop._h, kop._h if kop else None, n, k, _ptr(xb), ldx, _ptr(bb), ldb, float(tol), int(maxit),
                             info.ctypes.data_as(C.POINTER(C.c_int)), it.ctypes.data_as(C.POINTER(C.c_int)),
                             rr.ctypes.data_as(C.POINTER(C.c_double)))
    for op in (aop, kop):
        if op is not None and op.exc is not None:
            raise op.exc
    if rc == -1 and "multi-device" in lib().psp_last_error().decode():  # PSP_EINVAL
        raise ValueError("pcg_batch is not available on a multi-device matrix")
    check(rc)
    if copy_back:
        X[...] = xb
    return info, it, rr


def _solve_more(name, A, b, x, tol, maxit, K, dim=None):
    aop = _Op(A, "matvec")
    kop = _Op(K, "precon") if K is not None else None
    n = int(A.shape[0])
    xw = x if (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous
               and x.ndim == 1) else np.ascontiguousarray(x, dtype=np.float64)
    bw = np.ascontiguousarray(b, dtype=np.float64)
    if xw.ndim != 1 or bw.ndim != 1 or xw.shape[0] != bw.shape[0] or xw.shape[0] != n:
        raise ValueError("incompatible operand shapes")
    info, it, rr = C.c_int(0), C.c_int(0), C.c_double(0.0)
    fn = getattr(lib(), "psp_" + name)
    args = [aop._h, kop._h if kop else None, n, _ptr(xw), _ptr(bw), float(tol), int(maxit)]
    if dim is not None:
        args.append(int(dim))
    rc = fn(*args, C.byref(info), C.byref(it), C.byref(rr))
    for op in (aop, kop):
        if op is not None and op.exc is not None:
            raise op.exc
    check(rc)
    return info.value, it.value, rr.value


def cgs(A, b, x, tol, maxit, K=None):
    """info, iter, relres = cgs(A, b, x, tol, maxit[, K]) -- itsolversmodule.c:503-586."""
    return _solve_more("cgs", A, b, x, tol, maxit, K)


def bicgstab(A, b, x, tol, maxit, K=None):
    """info, iter, relres = bicgstab(A, b, x, tol, maxit[, K]) -- itsolversmodule.c:125-216."""
    return _solve_more("bicgstab", A, b, x, tol, maxit, K)


def qmrs(A, b, x, tol, maxit, K=None):
    """info, iter, relres = qmrs(A, b, x, tol, maxit[, K]) -- itsolversmodule.c:410-496."""
    return _solve_more("qmrs", A, b, x, tol, maxit, K)


def gmres(A, b, x, tol, maxit, K=None, dim=20):
    """info, iter, relres = gmres(A, b, x, tol, maxit[, K[, dim]]) -- itsolversmodule.c:313-403."""
    return _solve_more("gmres", A, b, x, tol, maxit, K, dim)


def last_solve_info():
    """(loop name, {launches, vec_bytes_per_row, dinv_streamed, single_kernel_fallbacks}) of the calling thread's last
    pcg / minres (psp_last_solve_info): which of the library's loops ran and what it moves per row beside its product."""
    name = C.create_string_buffer(64)
    info = (C.c_int * 4)()
    check(lib().psp_last_solve_info(name, 64, info))
    return name.value.decode(), {"launches": info[0], "vec_bytes_per_row": info[1], "dinv_streamed": bool(info[2]),
                                 "single_kernel_fallbacks": info[3]}


def set_single_kernel_loops(on):
    """psp_set_single_kernel_loops: False keeps every pcg / minres of this process on the launch-per-phase loops"""
    check(lib().psp_set_single_kernel_loops(1 if on else 0))


def device_count():
    return lib().psp_device_count()


def device_info():
    name = C.create_string_buffer(256)
    cu, mem = C.c_int(), C.c_int64()
    check(lib().psp_device_info(name, 256, C.byref(cu), C.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def debug_device_bytes():
    """(live_bytes, allocations): the device memory that precon.ssor / precon.multigrid handles and their set-up hold now
    through the library's owning array type -- and, while such a call runs, the staging of csr_mat's host-pointer diagonal
    and transposed product --, and the allocations that type has made so far (psp_debug_device_bytes)."""
    live, made = C.c_longlong(), C.c_longlong()
    check(lib().psp_debug_device_bytes(C.byref(live), C.byref(made)))
    return live.value, made.value
