"""pysparse_amd.eigen -- counterpart of pysparse.eigen: `jdsym.jdsym`, the Jacobi-Davidson eigensolver for symmetric
(generalised) eigenproblems, and `lobpcg.lobpcg`, the block eigensolver for their smallest eigenpairs; every n-vector on
the device."""
from . import jdsym  # noqa: F401
from . import lobpcg  # noqa: F401
