/*
 * pysparse_amd.precon.precon -- jacobi(A, omega=1.0, steps=1) and ssor(A, omega=1.0, steps=1):
 * objects with `shape` and `precon(x, y)` (pysparse/precon/src/preconmodule.c:11-80, 352-412,
 * 470-485 for jacobi; :21-31, 95-223, 414-459, 487-510 for ssor); multigrid(A, grid, omega=0.8, steps=2) has the
 * same shape and no reference analogue.
 *
 * dinv[i] = omega / A[i,i] lives on the GPU.  Native matrices hand over their diagonal on
 * the device (csr_mat / sss_mat; the reference can only subscript ll_mat, so jacobi(csr_mat)
 * is an extension); ll_mat and foreign objects are read through A[i,i] exactly like
 * newJacobiObject does (:389-401).
 */
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#define NPY_NO_DEPRECATED_API NPY_1_7_API_VERSION
#include <numpy/arrayobject.h>

#include <string.h>

#include "psp_pyops.h"

typedef struct {
  PyObject_VAR_HEAD
  int n;
  PyObject *matrix;
  double omega;
  int steps;
  psp_jacobi_t *dev;
  psp_op_t *op;    /* operator over dev, handed to the solvers */
  PyOpRef aref;    /* operator of the matrix (steps > 1 sweeps) */
  int have_aref;
} JacobiObject;

static PyTypeObject JacobiType;

static PyObject *raise_psp(int rc) {
  if (rc == PSP_ESINGULAR)
    PyErr_SetString(PyExc_ValueError, "diagonal element close to zero"); /* :396 */
  else if (rc == PSP_ENOMEM)
    PyErr_SetString(PyExc_MemoryError, psp_last_error());
  else if (rc == PSP_EINVAL)
    PyErr_SetString(PyExc_ValueError, psp_last_error());
  else
    PyErr_SetString(PyExc_RuntimeError, psp_last_error());
  return NULL;
}

static PyObject *newJacobiObject(PyObject *matrix, double omega, int steps) {
  JacobiObject *op;
  int n, rc, i;
  if (steps < 1) {
    PyErr_SetString(PyExc_ValueError, "steps must be >= 1");
    return NULL;
  }
  if (SpMatrix_GetOrder(matrix, &n)) return NULL;
  op = PyObject_New(JacobiObject, &JacobiType);
  if (op == NULL) return PyErr_NoMemory();
  op->n = n;
  op->matrix = NULL;
  op->omega = omega;
  op->steps = steps;
  op->dev = NULL;
  op->op = NULL;
  op->have_aref = 0;

  if (PyObject_TypeCheck(matrix, &CSRMatType)) {
    Py_BEGIN_ALLOW_THREADS
    rc = psp_jacobi_create_csr(((CSRMatObject *)matrix)->dev, omega, steps, &op->dev);
    Py_END_ALLOW_THREADS
  } else if (PyObject_TypeCheck(matrix, &SSSMatType)) {
    Py_BEGIN_ALLOW_THREADS
    rc = psp_jacobi_create_sss(((SSSMatObject *)matrix)->dev, omega, steps, &op->dev);
    Py_END_ALLOW_THREADS
  } else {
    double *diag = PyMem_New(double, n > 0 ? n : 1);
    int nn;
    if (diag == NULL) {
      Py_DECREF(op);
      return PyErr_NoMemory();
    }
    for (i = 0; i < n; i++) {
      if (PyObject_TypeCheck(matrix, &LLMatType))
        diag[i] = SpMatrix_LLMatGetItem((LLMatObject *)matrix, i, i);
      else
        diag[i] = SpMatrix_GetItem(matrix, i, i); /* :391 */
      if (PyErr_Occurred()) {
        PyMem_Del(diag);
        Py_DECREF(op);
        return NULL;
      }
    }
    if (steps > 1) {
      if (pyop_acquire(matrix, 0, &op->aref, &nn)) {
        PyMem_Del(diag);
        Py_DECREF(op);
        return NULL;
      }
      op->have_aref = 1;
    }
    Py_BEGIN_ALLOW_THREADS
    rc = psp_jacobi_create_diag(n, diag, omega, steps, op->have_aref ? op->aref.op : NULL, &op->dev);
    Py_END_ALLOW_THREADS
    PyMem_Del(diag);
  }
  if (rc != PSP_OK) {
    Py_DECREF(op);
    return raise_psp(rc);
  }
  Py_INCREF(matrix);
  op->matrix = matrix;
  return (PyObject *)op;
}

/* jacobi(A, omega=1.0, steps=1): preconmodule.c:470-485 */
static PyObject *jacobi_prec(PyObject *self, PyObject *args, PyObject *kw) {
  static char *kwlist[] = {"A", "omega", "steps", NULL};
  PyObject *matrix;
  double omega = 1.0;
  int steps = 1;
  if (!PyArg_ParseTupleAndKeywords(args, kw, "O|di", kwlist, &matrix, &omega, &steps)) return NULL;
  return newJacobiObject(matrix, omega, steps);
}

/* self.precon(x, y): Jacobi_precon, preconmodule.c:60-80 -- contiguous arrays only */
static PyObject *Jacobi_precon(JacobiObject *self, PyObject *args) {
  double *x, *y;
  int rc;
  if (SpMatrix_ParseVecOpArgs(args, &x, &y, self->n)) return NULL;
  Py_BEGIN_ALLOW_THREADS /* sweeps of a callback operator take the GIL back in pyop_trampoline */
  rc = psp_jacobi_precon(self->dev, x, y);
  Py_END_ALLOW_THREADS
  if (PyErr_Occurred()) return NULL;
  if (rc != PSP_OK) {
    PyErr_SetString(PyExc_RuntimeError, "unknown error in Jacobi iteration"); /* :74 */
    return NULL;
  }
  Py_RETURN_NONE;
}

static void Jacobi_dealloc(JacobiObject *self) {
  if (self->op) psp_op_destroy(self->op);
  if (self->dev) psp_jacobi_destroy(self->dev);
  if (self->have_aref) pyop_release(&self->aref);
  Py_XDECREF(self->matrix);
  PyObject_Del(self);
}

static PyObject *Jacobi_get_shape(JacobiObject *self, void *c) {
  return Py_BuildValue("(i,i)", self->n, self->n); /* :245-266 */
}

static PyObject *Jacobi_get_psp_op(JacobiObject *self, void *c) {
  if (self->op == NULL) {
    int rc = psp_op_from_jacobi(self->dev, &self->op);
    if (rc != PSP_OK) return raise_psp(rc);
  }
  return PyCapsule_New(self->op, PSP_OP_CAPSULE_NAME, NULL);
}

static PyMethodDef Jacobi_methods[] = {
    {"precon", (PyCFunction)Jacobi_precon, METH_VARARGS,
     "self.precon(x, y)\n\napply preconditioner self on x, store result in y. x is unchanged."},
    {NULL, NULL, 0, NULL}};

static PyGetSetDef Jacobi_getset[] = {{"shape", (getter)Jacobi_get_shape, NULL, "(n, n)", NULL},
                                      {"_psp_op", (getter)Jacobi_get_psp_op, NULL, "device operator", NULL},
                                      {NULL, NULL, NULL, NULL, NULL}};

/* ------------------------------------------------------------------------------ ssor */

typedef struct {
  PyObject_VAR_HEAD
  int n;
  PyObject *matrix; /* the sss_mat: the device handle borrows it */
  double omega;
  int steps;
  psp_ssor_t *dev;
  psp_op_t *op;
} SSORObject;

static PyTypeObject SSORType;

/* ssor(A, omega=1.0, steps=1): preconmodule.c:487-510 -- A must be an sss_mat ("O!") */
static PyObject *ssor_prec(PyObject *self, PyObject *args) {
  PyObject *matrix;
  double omega = 1.0;
  int steps = 1, n, rc;
  SSORObject *op;
  if (!PyArg_ParseTuple(args, "O!|di", &SSSMatType, &matrix, &omega, &steps)) return NULL;
  if (SpMatrix_GetOrder(matrix, &n)) return NULL; /* :421 */
  op = PyObject_New(SSORObject, &SSORType);
  if (op == NULL) return PyErr_NoMemory();
  op->n = n;
  op->matrix = NULL;
  op->omega = omega;
  op->steps = steps;
  op->dev = NULL;
  op->op = NULL;
  Py_BEGIN_ALLOW_THREADS
  rc = psp_ssor_create(((SSSMatObject *)matrix)->dev, omega, steps, &op->dev);
  Py_END_ALLOW_THREADS
  if (rc != PSP_OK) {
    Py_DECREF(op);
    return raise_psp(rc);
  }
  Py_INCREF(matrix);
  op->matrix = matrix;
  return (PyObject *)op;
}

/* self.precon(x, y): SSOR_precon, preconmodule.c:199-223 -- contiguous arrays only */
static PyObject *SSOR_precon(SSORObject *self, PyObject *args) {
  double *x, *y;
  int rc;
  if (SpMatrix_ParseVecOpArgs(args, &x, &y, self->n)) return NULL;
  Py_BEGIN_ALLOW_THREADS
  rc = psp_ssor_precon(self->dev, x, y);
  Py_END_ALLOW_THREADS
  if (rc != PSP_OK) return raise_psp(rc);
  Py_RETURN_NONE;
}

static void SSOR_dealloc(SSORObject *self) {
  if (self->op) psp_op_destroy(self->op);
  if (self->dev) psp_ssor_destroy(self->dev);
  Py_XDECREF(self->matrix);
  PyObject_Del(self);
}

static PyObject *SSOR_get_shape(SSORObject *self, void *c) {
  return Py_BuildValue("(i,i)", self->n, self->n); /* :297-318 */
}

static PyObject *SSOR_get_psp_op(SSORObject *self, void *c) {
  if (self->op == NULL) {
    int rc = psp_op_from_ssor(self->dev, &self->op);
    if (rc != PSP_OK) return raise_psp(rc);
  }
  return PyCapsule_New(self->op, PSP_OP_CAPSULE_NAME, NULL);
}

static PyMethodDef SSOR_methods[] = {
    {"precon", (PyCFunction)SSOR_precon, METH_VARARGS,
     "self.precon(x, y)\n\napply preconditioner self on x, store result in y. x is unchanged."},
    {NULL, NULL, 0, NULL}};

static PyGetSetDef SSOR_getset[] = {{"shape", (getter)SSOR_get_shape, NULL, "(n, n)", NULL},
                                    {"_psp_op", (getter)SSOR_get_psp_op, NULL, "device operator", NULL},
                                    {NULL, NULL, NULL, NULL, NULL}};


/* ------------------------------------------------------------------------- multigrid */

/* multigrid(A, grid, omega=0.8, steps=2, galerkin=False, precision='double', line=None): geometric V-cycle for the
 * constant-coefficient grid operators and, with the keyword galerkin=True (a real bool), for any symmetric 3- / 5- /
 * 7-point operator on the grid (psp_mg.hip); the keyword precision='single' (a str) selects the cycle evaluated in float32
 * (DESIGN.md 9g); the keyword line=a (an int, with galerkin=True) the line smoother along axis a for graded and
 * stretched grids; the keyword stencil='box' (a str, with galerkin=True) the 9- / 27-point operators
 * (DESIGN.md 9i); the keyword interp='operator' (a str, with galerkin=True) operator-dependent interpolation for jumping
 * coefficients; no reference analogue */
#define MG_MAX_LEVELS 40

typedef struct {
  PyObject_VAR_HEAD
  int n;
  int ndim;
  PyObject *matrix; /* kept for the caller's sake: the handle reads it at creation only */
  psp_mg_t *dev;
  psp_op_t *op;
} MGObject;

static PyTypeObject MGType;

static PyObject *multigrid_prec(PyObject *self, PyObject *args, PyObject *kw) {
  static char *kwlist[] = {"A", "grid", "omega", "steps", "galerkin", "precision", "line", "stencil", "interp", NULL};
  PyObject *matrix, *grid, *seq, *cap, *galerkin_obj = Py_False, *precision_obj = NULL, *line_obj = Py_None;
  PyObject *stencil_obj = NULL, *interp_obj = NULL;
  int galerkin;
  long line = -1;
  unsigned flags = 0;
  double omega = 0.8;
  int steps = 2, ndim, a, rc, shape[2], dims[3] = {1, 1, 1};
  int is_csr, is_sss, is_ll;
  long long prod = 1;
  MGObject *op;
  if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|di$OOOOO", kwlist, &matrix, &grid, &omega, &steps, &galerkin_obj,
                                   &precision_obj, &line_obj, &stencil_obj, &interp_obj))
    return NULL;
  if (!PyBool_Check(galerkin_obj)) {
    PyErr_SetString(PyExc_TypeError, "multigrid() argument 'galerkin' must be a bool");
    return NULL;
  }
  galerkin = galerkin_obj == Py_True;
  if (galerkin) flags |= PSP_MG_GALERKIN;
  if (precision_obj != NULL) { /* exactly the str 'double' or 'single' */
    if (!PyUnicode_Check(precision_obj)) {
      PyErr_SetString(PyExc_TypeError, "multigrid() argument 'precision' must be a str, 'double' or 'single'");
      return NULL;
    }
    if (PyUnicode_CompareWithASCIIString(precision_obj, "single") == 0)
      flags |= PSP_MG_SINGLE;
    else if (PyUnicode_CompareWithASCIIString(precision_obj, "double") != 0) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'precision' must be 'double' or 'single'");
      return NULL;
    }
  }
  if (stencil_obj != NULL) { /* exactly the str 'axis' or 'box'  */
    if (!PyUnicode_Check(stencil_obj)) {
      PyErr_SetString(PyExc_TypeError, "multigrid() argument 'stencil' must be a str, 'axis' or 'box'");
      return NULL;
    }
    if (PyUnicode_CompareWithASCIIString(stencil_obj, "box") == 0) {
      if (!galerkin) {
        PyErr_SetString(PyExc_ValueError, "multigrid() argument 'stencil': 'box' needs galerkin=True: the matrix-free mode "
                                          "stores no level operators");
        return NULL;
      }
      if (line_obj != Py_None) {
        PyErr_SetString(PyExc_ValueError, "multigrid() argument 'stencil': 'box' with line is not supported");
        return NULL;
      }
      flags |= PSP_MG_BOX;
    } else if (PyUnicode_CompareWithASCIIString(stencil_obj, "axis") != 0) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'stencil' must be 'axis' or 'box'");
      return NULL;
    }
  }
  if (line_obj != Py_None) { /* an int (no bool), the axis of the line smoother */
    if (PyBool_Check(line_obj) || !PyLong_Check(line_obj)) {
      PyErr_SetString(PyExc_TypeError, "multigrid() argument 'line' must be None or an int, the axis of the line smoother");
      return NULL;
    }
    line = PyLong_AsLong(line_obj);
    if (line == -1 && PyErr_Occurred()) {
      PyErr_Clear();
      line = -2; /* out of every range */
    }
    if (!galerkin) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'line' needs galerkin=True: the line smoother works on stored "
                                        "level operators");
      return NULL;
    }
    if (flags & PSP_MG_SINGLE) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'line' with precision='single': the line smoother has no "
                                        "single-precision form");
      return NULL;
    }
  }
  if (interp_obj != NULL) { /* exactly the str 'linear' or 'operator'  */
    if (!PyUnicode_Check(interp_obj)) {
      PyErr_SetString(PyExc_TypeError, "multigrid() argument 'interp' must be a str, 'linear' or 'operator'");
      return NULL;
    }
    if (PyUnicode_CompareWithASCIIString(interp_obj, "operator") == 0) {
      if (!galerkin) {
        PyErr_SetString(PyExc_ValueError, "multigrid() argument 'interp': 'operator' needs galerkin=True: the weights come "
                                          "from stored level operators");
        return NULL;
      }
      if (line_obj != Py_None) {
        PyErr_SetString(PyExc_ValueError, "multigrid() argument 'interp': 'operator' with line is not supported");
        return NULL;
      }
      if (flags & PSP_MG_SINGLE) {
        PyErr_SetString(PyExc_ValueError, "multigrid() argument 'interp': 'operator' with precision='single' is not supported");
        return NULL;
      }
      flags |= PSP_MG_INTERP;
    } else if (PyUnicode_CompareWithASCIIString(interp_obj, "linear") != 0) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'interp' must be 'linear' or 'operator'");
      return NULL;
    }
  }
  is_csr = PyObject_TypeCheck(matrix, &CSRMatType);
  is_sss = PyObject_TypeCheck(matrix, &SSSMatType);
  is_ll = PyObject_TypeCheck(matrix, &LLMatType);
  if (!is_csr && !is_sss && !is_ll) {
    PyErr_SetString(PyExc_TypeError, "multigrid() argument 1 must be csr_mat, sss_mat or ll_mat");
    return NULL;
  }
  if (!PySequence_Check(grid) || PyUnicode_Check(grid) || PyBytes_Check(grid)) {
    PyErr_SetString(PyExc_TypeError, "multigrid() argument 2 must be a sequence of 1 to 3 positive integers");
    return NULL;
  }
  seq = PySequence_Fast(grid, "multigrid() argument 2 must be a sequence of 1 to 3 positive integers");
  if (seq == NULL) return NULL;
  ndim = (int)PySequence_Fast_GET_SIZE(seq);
  if (ndim < 1 || ndim > 3) {
    Py_DECREF(seq);
    PyErr_SetString(PyExc_ValueError, "grid must have 1 to 3 axes");
    return NULL;
  }
  for (a = 0; a < ndim; a++) {
    long v = PyLong_AsLong(PySequence_Fast_GET_ITEM(seq, a));
    if (v == -1 && PyErr_Occurred()) {
      Py_DECREF(seq);
      return NULL; /* TypeError of a non-integer, OverflowError */
    }
    if (v < 1 || v > 0x7fffffffL) {
      Py_DECREF(seq);
      PyErr_SetString(PyExc_ValueError, "grid axes must be positive integers");
      return NULL;
    }
    dims[a] = (int)v;
    prod *= v;
    if (prod > 0x7fffffffLL) prod = 0x80000000LL; /* matches no matrix order */
  }
  Py_DECREF(seq);
  if (line_obj != Py_None) {
    if (ndim < 2) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'line' on a grid of one axis: there is no axis left to coarsen");
      return NULL;
    }
    if (line < 0 || line >= ndim) {
      PyErr_Format(PyExc_ValueError, "multigrid() argument 'line' must be one of the grid's axes, 0 .. %d", ndim - 1);
      return NULL;
    }
    if (dims[line] < 2) {
      PyErr_SetString(PyExc_ValueError, "multigrid() argument 'line': the line axis must have at least 2 points");
      return NULL;
    }
  }
  if (SpMatrix_GetShape(matrix, shape)) return NULL;
  if (shape[0] != shape[1]) {
    PyErr_SetString(PyExc_ValueError, "matrix is not square");
    return NULL;
  }
  if (prod != (long long)shape[0]) {
    PyErr_SetString(PyExc_ValueError, "prod(grid) does not match the matrix order");
    return NULL;
  }
  if (!(omega > 0.0 && omega <= 1.0)) {
    PyErr_SetString(PyExc_ValueError, "omega must satisfy 0 < omega <= 1");
    return NULL;
  }
  if (steps < 1) {
    PyErr_SetString(PyExc_ValueError, "steps must be >= 1");
    return NULL;
  }
  if (is_ll) { /* the device mirror of the linked list is built by the operator getter */
    cap = PyObject_GetAttrString(matrix, "_psp_op");
    if (cap == NULL) return NULL;
    Py_DECREF(cap);
    if (((LLMatObject *)matrix)->mirror == NULL) {
      PyErr_SetString(PyExc_RuntimeError, "ll_mat has no device mirror");
      return NULL;
    }
  }
  op = PyObject_New(MGObject, &MGType);
  if (op == NULL) return PyErr_NoMemory();
  op->n = shape[0];
  op->ndim = ndim;
  op->matrix = NULL;
  op->dev = NULL;
  op->op = NULL;
  Py_BEGIN_ALLOW_THREADS
  if (line_obj != Py_None && is_sss)
    rc = psp_mg_create_sss_line(((SSSMatObject *)matrix)->dev, ndim, dims, omega, steps, (int)line, &op->dev);
  else if (line_obj != Py_None)
    rc = psp_mg_create_csr_line(is_csr ? ((CSRMatObject *)matrix)->dev : ((LLMatObject *)matrix)->mirror, ndim, dims, omega,
                                steps, (int)line, &op->dev);
  else if (is_sss)
    rc = psp_mg_create_sss_ex(((SSSMatObject *)matrix)->dev, ndim, dims, omega, steps, flags, &op->dev);
  else
    rc = psp_mg_create_csr_ex(is_csr ? ((CSRMatObject *)matrix)->dev : ((LLMatObject *)matrix)->mirror, ndim, dims, omega,
                              steps, flags, &op->dev);
  Py_END_ALLOW_THREADS
  if (rc != PSP_OK) {
    Py_DECREF(op);
    return raise_psp(rc);
  }
  Py_INCREF(matrix);
  op->matrix = matrix;
  return (PyObject *)op;
}

/* self.precon(x, y): one V-cycle -- contiguous arrays only */
static PyObject *MG_precon(MGObject *self, PyObject *args) {
  double *x, *y;
  int rc;
  if (SpMatrix_ParseVecOpArgs(args, &x, &y, self->n)) return NULL;
  Py_BEGIN_ALLOW_THREADS
  rc = psp_mg_precon(self->dev, x, y);
  Py_END_ALLOW_THREADS
  if (rc != PSP_OK) return raise_psp(rc);
  Py_RETURN_NONE;
}

/* self.precon_block(X, Y): Y[:, c] := K X[:, c] for every column in one block cycle (psp_mg_precon_block).  X and Y are
 * (n, k) double arrays with any strides, staged as column-major blocks like a.matmat(X, Y); Y is written back in place. */
static PyObject *MG_precon_block(MGObject *self, PyObject *args) {
  PyArrayObject *xp, *yp, *xf = NULL, *yf = NULL;
  PyObject *result = NULL;
  npy_intp dims[2];
  int rc, k;
  if (!PyArg_ParseTuple(args, "O!O!", &PyArray_Type, &xp, &PyArray_Type, &yp)) return NULL;
  if (PyArray_NDIM(xp) != 2 || PyArray_TYPE(xp) != NPY_DOUBLE || PyArray_DIM(xp, 0) != self->n || PyArray_DIM(xp, 1) < 1 ||
      PyArray_DIM(xp, 1) > 0x7fffffff) {
    PyErr_SetString(PyExc_ValueError, "arg 1 must be a 2-dimensional double array of appropriate size.");
    return NULL;
  }
  if (PyArray_NDIM(yp) != 2 || PyArray_TYPE(yp) != NPY_DOUBLE || PyArray_DIM(yp, 0) != self->n ||
      PyArray_DIM(yp, 1) != PyArray_DIM(xp, 1)) {
    PyErr_SetString(PyExc_ValueError, "arg 2 must be a 2-dimensional double array of appropriate size.");
    return NULL;
  }
  if (!PyArray_ISWRITEABLE(yp)) {
    PyErr_SetString(PyExc_ValueError, "arg 2 must be writeable.");
    return NULL;
  }
  k = (int)PyArray_DIM(xp, 1);
  xf = (PyArrayObject *)PyArray_FromArray(xp, NULL, NPY_ARRAY_F_CONTIGUOUS | NPY_ARRAY_ALIGNED);
  dims[0] = self->n;
  dims[1] = k;
  yf = (PyArrayObject *)PyArray_EMPTY(2, dims, NPY_DOUBLE, 1); /* never X's memory: the cycle is out of place */
  if (!xf || !yf) goto done;
  Py_BEGIN_ALLOW_THREADS
  rc = psp_mg_precon_block(self->dev, k, (const double *)PyArray_DATA(xf), (long)self->n, (double *)PyArray_DATA(yf),
                           (long)self->n);
  Py_END_ALLOW_THREADS
  if (rc != PSP_OK) {
    raise_psp(rc);
    goto done;
  }
  if (PyArray_CopyInto(yp, yf) < 0) goto done;
  result = Py_None;
  Py_INCREF(result);
done:
  Py_XDECREF(xf);
  Py_XDECREF(yf);
  return result;
}

static void MG_dealloc(MGObject *self) {
  if (self->op) psp_op_destroy(self->op);
  if (self->dev) psp_mg_destroy(self->dev);
  Py_XDECREF(self->matrix);
  PyObject_Del(self);
}

static PyObject *MG_get_shape(MGObject *self, void *c) { return Py_BuildValue("(i,i)", self->n, self->n); }

static PyObject *MG_get_psp_op(MGObject *self, void *c) {
  if (self->op == NULL) {
    int rc = psp_op_from_mg(self->dev, &self->op);
    if (rc != PSP_OK) return raise_psp(rc);
  }
  return PyCapsule_New(self->op, PSP_OP_CAPSULE_NAME, NULL);
}

/* the level grids, finest first: a tuple of tuples with as many entries as `grid` had */
static PyObject *MG_get_levels(MGObject *self, void *c) {
  int levels = 0, l, a, rc, dims[3 * MG_MAX_LEVELS];
  PyObject *out;
  rc = psp_mg_info(self->dev, &levels, NULL, NULL, NULL);
  if (rc != PSP_OK) return raise_psp(rc);
  if (levels > MG_MAX_LEVELS) {
    PyErr_SetString(PyExc_RuntimeError, "too many levels");
    return NULL;
  }
  rc = psp_mg_info(self->dev, NULL, NULL, NULL, dims);
  if (rc != PSP_OK) return raise_psp(rc);
  out = PyTuple_New(levels);
  if (out == NULL) return NULL;
  for (l = 0; l < levels; l++) {
    PyObject *t = PyTuple_New(self->ndim);
    if (t == NULL) {
      Py_DECREF(out);
      return NULL;
    }
    for (a = 0; a < self->ndim; a++) PyTuple_SET_ITEM(t, a, PyLong_FromLong(dims[3 * l + a]));
    PyTuple_SET_ITEM(out, l, t);
  }
  return out;
}

static PyObject *MG_get_galerkin(MGObject *self, void *c) {
  int g = 0, rc = psp_mg_is_galerkin(self->dev, &g);
  if (rc != PSP_OK) return raise_psp(rc);
  return PyBool_FromLong(g);
}

static PyObject *MG_get_precision(MGObject *self, void *c) {
  int bits = 0, rc = psp_mg_precision(self->dev, &bits);
  if (rc != PSP_OK) return raise_psp(rc);
  return PyUnicode_FromString(bits == 32 ? "single" : "double");
}

/* 'axis', or 'box' for a handle that takes 9- / 27-point operators */
static PyObject *MG_get_stencil(MGObject *self, void *c) {
  int box = 0, rc = psp_mg_stencil(self->dev, &box);
  if (rc != PSP_OK) return raise_psp(rc);
  return PyUnicode_FromString(box ? "box" : "axis");
}

/* 'linear', or 'operator' for a handle with operator-dependent interpolation */
static PyObject *MG_get_interp(MGObject *self, void *c) {
  int op = 0, rc = psp_mg_interp(self->dev, &op);
  if (rc != PSP_OK) return raise_psp(rc);
  return PyUnicode_FromString(op ? "operator" : "linear");
}

/* the axis of the line smoother, None without one */
static PyObject *MG_get_line(MGObject *self, void *c) {
  int axis = -1, rc = psp_mg_line_axis(self->dev, &axis);
  if (rc != PSP_OK) return raise_psp(rc);
  if (axis < 0) Py_RETURN_NONE;
  return PyLong_FromLong(axis);
}

static PyMethodDef MG_methods[] = {
    {"precon", (PyCFunction)MG_precon, METH_VARARGS,
     "self.precon(x, y)\n\napply preconditioner self on x, store result in y. x is unchanged."},
    {"precon_block", (PyCFunction)MG_precon_block, METH_VARARGS,
     "self.precon_block(X, Y)\n\nY[:, c] := K X[:, c] for every column of the (n, k) arrays in one block cycle; column c has "
     "the bits of precon on X[:, c]. X is unchanged."},
    {NULL, NULL, 0, NULL}};

static PyGetSetDef MG_getset[] = {{"shape", (getter)MG_get_shape, NULL, "(n, n)", NULL},
                                  {"levels", (getter)MG_get_levels, NULL, "the level grids, finest first", NULL},
                                  {"galerkin", (getter)MG_get_galerkin, NULL, "stored Galerkin level operators", NULL},
                                  {"precision", (getter)MG_get_precision, NULL, "'double' or 'single'", NULL},
                                  {"line", (getter)MG_get_line, NULL, "the axis of the line smoother, or None", NULL},
                                  {"stencil", (getter)MG_get_stencil, NULL, "'axis' or 'box'", NULL},
                                  {"interp", (getter)MG_get_interp, NULL, "'linear' or 'operator'", NULL},
                                  {"_psp_op", (getter)MG_get_psp_op, NULL, "device operator", NULL},
                                  {NULL, NULL, NULL, NULL, NULL}};

static PyMethodDef precon_methods[] = {
    {"jacobi", (PyCFunction)jacobi_prec, METH_VARARGS | METH_KEYWORDS,
     "jacobi(A, omega=1.0, steps=1)\n\nnew Jacobi preconditioner object"},
    {"ssor", (PyCFunction)ssor_prec, METH_VARARGS,
     "ssor(A, omega, steps) -- return SSOR preconditioner object\n\n"
     "This preconditioner executes 'steps' SSOR steps with a zero initial guess.\n\n"
     "A      'sss_mat' object, symmetric sparse matrix\n"
     "omega  relaxation parameter (default value: 1.0)\n"
     "steps  number of SSOR steps"},
    {"multigrid", (PyCFunction)multigrid_prec, METH_VARARGS | METH_KEYWORDS,
     "multigrid(A, grid, omega=0.8, steps=2, galerkin=False, precision='double', line=None, stencil='axis',\n"
     "interp='linear') -- return\n"
     "geometric multigrid\n"
     "preconditioner object\n\n"
     "One V-cycle with damped-Jacobi smoothing for A = sum_a c_a T_a + s I on a grid (no reference analogue).\n\n"
     "A      'csr_mat', 'sss_mat' or 'll_mat': the constant-coefficient [-1 2 -1] stencil on the grid\n"
     "grid   (n0[, n1[, n2]]), prod(grid) == n, row k = i0 + n0*i1 + n0*n1*i2\n"
     "omega  damping of the Jacobi sweeps, 0 < omega <= 1 (default value: 0.8)\n"
     "steps  sweeps before and after the coarse-grid correction (default value: 2)\n"
     "galerkin  keyword, a bool: True takes any symmetric 3- / 5- / 7-point operator on the grid (varying\n"
     "       coefficients) and stores the level operators R A P (default value: False)\n"
     "precision  keyword, a str: 'single' runs the cycle in float32 on level operators rounded once from the\n"
     "       double ones; x and y stay double arrays, the outer solver is unchanged (default value: 'double')\n"
     "line   keyword, None or an int: with galerkin=True, the grid axis along which the cells are graded or stretched;\n"
     "       that axis is never coarsened and the smoother solves the level operator's tridiagonal part along each of\n"
     "       its grid lines exactly instead of point Jacobi; double precision only (default value: None)\n"
     "stencil  keyword, a str: 'box' (with galerkin=True, without line) takes any symmetric operator with the pattern\n"
     "       {-1, 0, 1}^ndim, 9 points in 2-D and 27 in 3-D (default value: 'axis')\n"
     "interp  keyword, a str: 'operator' (with galerkin=True, without line, double precision) derives the interpolation\n"
     "       weights of every level from the level operator's own stencil, for coefficients that jump between regions\n"
     "       (default value: 'linear').  Rule of thumb: it pays while the regions are still a few cells wide after\n"
     "       most of the coarsenings, i.e. on grids of up to about 16 regions a side; where the regions are small\n"
     "       against the grid (8-cell blocks on 4096 x 4096: 1565 iterations against 160) keep 'linear'"},
    {NULL, NULL, 0, NULL}};

static struct PyModuleDef precon_module = {PyModuleDef_HEAD_INIT, "precon",
                                           "preconditioners on MI355X", -1, precon_methods,
                                           NULL, NULL, NULL, NULL};

PyMODINIT_FUNC PyInit_precon(void) {
  PyObject *m;
  import_array();
  if (import_spmatrix() < 0) return NULL;
  {
    PyTypeObject zero = {PyVarObject_HEAD_INIT(NULL, 0)};
    JacobiType = zero;
  }
  JacobiType.tp_name = "pysparse_amd.precon.precon.jacobi";
  JacobiType.tp_basicsize = sizeof(JacobiObject);
  JacobiType.tp_dealloc = (destructor)Jacobi_dealloc;
  JacobiType.tp_flags = Py_TPFLAGS_DEFAULT;
  JacobiType.tp_methods = Jacobi_methods;
  JacobiType.tp_getset = Jacobi_getset;
  if (PyType_Ready(&JacobiType) < 0) return NULL;
  {
    PyTypeObject zero = {PyVarObject_HEAD_INIT(NULL, 0)};
    SSORType = zero;
  }
  SSORType.tp_name = "pysparse_amd.precon.precon.ssor";
  SSORType.tp_basicsize = sizeof(SSORObject);
  SSORType.tp_dealloc = (destructor)SSOR_dealloc;
  SSORType.tp_flags = Py_TPFLAGS_DEFAULT;
  SSORType.tp_methods = SSOR_methods;
  SSORType.tp_getset = SSOR_getset;
  if (PyType_Ready(&SSORType) < 0) return NULL;
  {
    PyTypeObject zero = {PyVarObject_HEAD_INIT(NULL, 0)};
    MGType = zero;
  }
  MGType.tp_name = "pysparse_amd.precon.precon.multigrid";
  MGType.tp_basicsize = sizeof(MGObject);
  MGType.tp_dealloc = (destructor)MG_dealloc;
  MGType.tp_flags = Py_TPFLAGS_DEFAULT;
  MGType.tp_methods = MG_methods;
  MGType.tp_getset = MG_getset;
  if (PyType_Ready(&MGType) < 0) return NULL;
  m = PyModule_Create(&precon_module);
  if (m == NULL) return NULL;
  Py_INCREF(&JacobiType);
  PyModule_AddObject(m, "JacobiType", (PyObject *)&JacobiType);
  Py_INCREF(&SSORType);
  PyModule_AddObject(m, "SSORType", (PyObject *)&SSORType);
  Py_INCREF(&MGType);
  PyModule_AddObject(m, "MultigridType", (PyObject *)&MGType);
  return m;
}
