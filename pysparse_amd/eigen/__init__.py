"""pysparse_amd.eigen -- counterpart of pysparse.eigen: `jdsym.jdsym`, the Jacobi-Davidson eigensolver for symmetric
(generalised) eigenproblems, every n-vector on the device."""
from . import jdsym  # noqa: F401
