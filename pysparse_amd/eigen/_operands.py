"""pysparse_amd.eigen._operands -- how the eigensolvers (jdsym, lobpcg) take their operands: a native object through its
`_psp_op` capsule, anything else with `shape` and `matvec` / `precon` through a host-callback operator."""
import ctypes as C

import numpy as np

from .. import _capi

_CAPSULE = b"psp_op_t"
_capsule_is_valid = C.pythonapi.PyCapsule_IsValid
_capsule_is_valid.restype = C.c_int
_capsule_is_valid.argtypes = [C.py_object, C.c_char_p]
_capsule_pointer = C.pythonapi.PyCapsule_GetPointer
_capsule_pointer.restype = C.c_void_p
_capsule_pointer.argtypes = [C.py_object, C.c_char_p]


def _order(obj, what):
    try:
        shape = tuple(obj.shape)
    except (AttributeError, TypeError):
        raise ValueError("%s has no shape" % what)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("%s is not square" % what)
    return int(shape[0])


def _raise(rc):
    msg = _capi.lib().psp_last_error().decode()
    if rc == -1:  # PSP_EINVAL
        raise ValueError(msg)
    if rc == -3:
        raise MemoryError(msg)
    raise _capi.PspError(rc, msg)


class _Operator(object):
    """a psp_op_t for `obj`: the object's own handle, or a host-callback operator over obj.matvec / obj.precon"""

    def __init__(self, obj, n, precon):
        self.ptr = None
        self.owned = False
        self.error = None
        cap = getattr(obj, "_psp_op", None)  # native getters raise what the library reports (no HIP device, ...)
        if cap is not None and _capsule_is_valid(cap, _CAPSULE):
            self.keep = cap
            self.ptr = _capsule_pointer(cap, _CAPSULE)
            return
        method = getattr(obj, "precon" if precon else "matvec", None)
        if method is None:
            raise TypeError("object has neither a device handle nor a %s method" % ("precon" if precon else "matvec"))

        def apply(ctx, nn, xp, yp):
            try:
                method(np.ctypeslib.as_array(xp, (nn,)), np.ctypeslib.as_array(yp, (nn,)))
                return 0
            except BaseException as e:  # noqa: B902 -- handed to the solver's caller once the library has returned
                self.error = e
                return 1

        self.fn = _capi.HOST_APPLY_FN(apply)
        out = C.c_void_p()
        rc = _capi.lib().psp_op_from_callback(n, self.fn, None, C.byref(out))
        if rc != 0:
            _raise(rc)
        self.ptr = out.value
        self.owned = True

    def close(self):
        if self.owned and self.ptr:
            _capi.lib().psp_op_destroy(self.ptr)
        self.ptr = None
