"""CPU: argument validation of matmat / pcg_batch that is reached before any device call -- the drop-in modules'
ll_mat.matmat and krylov.pcg_batch and the ctypes layer's pcg_batch -- and the presence of both in the alias package.
Nothing here needs a GPU."""
import numpy as np
import pytest


def ll(n, m=None):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, m or n)
    for i in range(min(n, m or n)):
        A[i, i] = 2.0
    return A


def test_alias_package_exposes_both():
    from pysparse.itsolvers import krylov
    from pysparse.sparse import spmatrix
    import pysparse_amd.itsolvers.krylov as k2
    assert callable(krylov.pcg_batch) and krylov.pcg_batch is k2.pcg_batch
    assert hasattr(spmatrix.ll_mat(2, 2), "matmat")
    from pysparse_amd import device
    assert callable(device.pcg_batch) and hasattr(device.DeviceCSR, "matmat") and hasattr(device.DeviceSSS, "matmat")


@pytest.mark.parametrize("X,Y,exc", [
    (np.ones((7, 2)), np.zeros((5, 2)), ValueError),           # rows of X
    (np.ones((6, 2)), np.zeros((6, 2)), ValueError),           # rows of Y
    (np.ones((6, 2)), np.zeros((5, 3)), ValueError),           # column counts differ
    (np.ones(6), np.zeros(5), ValueError),                     # vectors are matvec's
    (np.ones((6, 0)), np.zeros((5, 0)), ValueError),           # no column
    (np.ones((6, 2), dtype=np.float32), np.zeros((5, 2)), ValueError),
    (np.ones((6, 2)), np.zeros((5, 2), dtype=np.int64), ValueError),
    ([[1.0, 1.0]] * 6, np.zeros((5, 2)), TypeError),
    (np.ones((6, 2)), [[0.0, 0.0]] * 5, TypeError),
])
def test_ll_mat_matmat_refuses(X, Y, exc):
    A = ll(5, 6)
    with pytest.raises(exc):
        A.matmat(X, Y)


def test_ll_mat_matmat_refuses_read_only_result():
    A = ll(5, 6)
    Y = np.zeros((5, 2))
    Y.flags.writeable = False
    with pytest.raises(ValueError):
        A.matmat(np.ones((6, 2)), Y)


def test_krylov_pcg_batch_refuses_before_any_device_call():
    from pysparse.itsolvers import krylov
    A = ll(5)
    with pytest.raises(TypeError):
        krylov.pcg_batch(A, [[1.0, 1.0]] * 5, np.zeros((5, 2)), 1e-8, 10)
    with pytest.raises(TypeError):
        krylov.pcg_batch(A, np.ones((5, 2)), [[0.0, 0.0]] * 5, 1e-8, 10)
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((5, 2), dtype=np.float32), np.zeros((5, 2)), 1e-8, 10)
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((5, 2)), np.zeros((5, 2), dtype=np.float32), 1e-8, 10)
    X = np.zeros((5, 2))
    X.flags.writeable = False
    with pytest.raises(ValueError):
        krylov.pcg_batch(A, np.ones((5, 2)), X, 1e-8, 10)
    with pytest.raises(TypeError):
        krylov.pcg_batch(A, np.ones((5, 2)))


def test_device_layer_pcg_batch_refuses_before_any_device_call():
    from pysparse_amd.device import pcg_batch

    class Shape:
        shape = (5, 5)

    A = Shape()
    with pytest.raises(TypeError):
        pcg_batch(A, [[1.0, 1.0]] * 5, np.zeros((5, 2)), 1e-8, 10)
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones((5, 2)), np.zeros((5, 3)), 1e-8, 10)
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones((6, 2)), np.zeros((6, 2)), 1e-8, 10)
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones(5), np.zeros(5), 1e-8, 10)
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones((5, 0)), np.zeros((5, 0)), 1e-8, 10)
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones((5, 2), dtype=np.float32), np.zeros((5, 2)), 1e-8, 10)
    X = np.zeros((5, 2))
    X.flags.writeable = False
    with pytest.raises(ValueError):
        pcg_batch(A, np.ones((5, 2)), X, 1e-8, 10)


def test_block_staging_of_the_device_layer():
    """_block hands column-major blocks over as they are and copies everything else"""
    from pysparse_amd.device import _block
    F = np.zeros((9, 4), order="F")
    a, ld, copied = _block(F[:6, 1:3], 6, "X")
    assert not copied and ld == 9 and a.ctypes.data == F[:6, 1:3].ctypes.data
    a, ld, copied = _block(np.zeros((6, 3)), 6, "X")
    assert copied and ld == 6 and a.flags.f_contiguous
    a, ld, copied = _block(F[::2, :], 5, "X")
    assert copied and ld == 5
    a, ld, copied = _block(np.zeros((6, 1)), 6, "X")
    assert ld == 6
    with pytest.raises(ValueError):
        _block(np.zeros((6, 3)), 5, "X")
    with pytest.raises(TypeError):
        _block([[0.0]], 1, "X")
