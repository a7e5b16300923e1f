"""GPU: the block-vector kernels behind pysparse.eigen.lobpcg through the C ABI -- psp_bv_gram (G = A' B with a register
tile per thread) and psp_bv_resid (R = AX - theta MX, its norms and the compaction of the active columns in one pass).

Contracts.  gram: column b of G has the bits of psp_bv_tdot(n, ma, A, lda, B + b ldb, h) whenever the two
kernels take the same access form for that column -- both leading dimensions even, or n odd; in the mixed cases (and
always, against np.longdouble) the project's dot-product bound 4 sqrt(n) eps ||A_a|| ||B_b|| holds.  resid: R is what
NumPy gives for AX - theta * MX evaluated in that order (product rounded, then the difference), nrm2 has the bits of
psp_bv_tdot of the stored column with itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NS = [1, 63, 64, 65, 1023, 4097, 65539]
FOLD_NS = [131073, 131074, 1 << 20]
SHAPES = [(1, 1), (3, 5), (8, 4), (9, 9), (24, 24), (33, 7)]


def lib():
    from pysparse_amd import _capi
    return _capi.lib()


def buf(a):
    from pysparse_amd import device
    return device.DeviceBuffer.from_host(np.ascontiguousarray(a, dtype=np.float64))


def block(rng, n, m, ld):
    """column-major n x m block of leading dimension ld, padding rows NaN: (flat storage, n x m view of the values)"""
    store = np.full((max(m, 1), ld), np.nan)
    store[:m, :n] = rng.standard_normal((m, n))
    return store, store[:m, :n].T


def lds(n):
    return [n, n + 5, n + 6]


def tdot(L, n, m, dV, ld, dx_ptr):
    dh = buf(np.full(m, np.nan))
    assert L.psp_bv_tdot(n, m, dV.ptr, ld, dx_ptr, dh.ptr) == 0, L.psp_last_error()
    return dh.download()


def gram(L, n, ma, dA, lda, mb, dB, ldb, ldg):
    dG = buf(np.full((mb + 1, ldg), np.nan))
    assert L.psp_bv_gram(n, ma, dA.ptr, lda, mb, dB.ptr, ldb, dG.ptr, ldg) == 0, L.psp_last_error()
    return dG.download().reshape(mb + 1, ldg)  # [b, a]


def pack(vals, ld):
    """the n x m values as a column-major block of leading dimension ld with NaN padding rows"""
    n, m = vals.shape
    store = np.full((m, ld), np.nan)
    store[:, :n] = vals.T
    return store


def check_gram(n, shapes, ld_pairs, seed):
    L = lib()
    rng = np.random.default_rng(seed)
    worst, exact = 0.0, 0
    for ma, mb in shapes:
        A, B = rng.standard_normal((n, ma)), rng.standard_normal((n, mb))
        ref = (A.astype(LD).T @ B.astype(LD)).astype(np.float64)
        bound = 4 * np.sqrt(n) * EPS * np.outer(np.linalg.norm(A, axis=0), np.linalg.norm(B, axis=0))
        for lda, ldb in ld_pairs:
            dA, dB = buf(pack(A, lda)), buf(pack(B, ldb))
            ldg = ma + 3
            G = gram(L, n, ma, dA, lda, mb, dB, ldb, ldg)
            assert np.array_equal(G, gram(L, n, ma, dA, lda, mb, dB, ldb, ldg), equal_nan=True), "two runs differ"
            assert np.all(np.isnan(G[:mb, ma:])) and np.all(np.isnan(G[mb])), "wrote outside the ma x mb entries"
            got = G[:mb, :ma].T  # [a, b]
            err = np.abs(got - ref)
            worst = max(worst, (err / bound).max())
            assert np.all(err <= bound), (n, ma, mb, lda, ldb, (err / bound).max())
            if (lda % 2 == 0 and ldb % 2 == 0) or n % 2 == 1:  # the same access form in both kernels, every column
                for b in range(mb):
                    h = tdot(L, n, ma, dA, lda, C.c_void_p(dB.ptr + 8 * b * ldb))
                    assert np.array_equal(got[:, b], h), (n, ma, mb, lda, ldb, b)
                exact += 1
    return worst, exact


@pytest.mark.parametrize("n", NS)
def test_gram(n):
    pairs = [(n, n), (n + 6, n + 6), (n + 5, n + 6), (n + 6, n + 5), (n + 5, n + 5), (n, n + 6)]
    worst, exact = check_gram(n, SHAPES, pairs, n)
    assert exact >= len(SHAPES)
    print("gram n=%d: worst error / bound %.3f, %d shape x ld cases bit-equal to tdot" % (n, worst, exact))


@pytest.mark.parametrize("n", FOLD_NS)
def test_gram_two_level_fold(n):
    """more than 256 workgroup sums per entry: the finishing block adds groups of 256, then the group sums"""
    assert (n + 511) // 512 > 256
    worst, exact = check_gram(n, [(3, 5), (9, 9)], [(n, n), (n + 6, n + 5), (n + 6, n + 6)], n)
    assert exact >= 2
    print("gram n=%d: worst error / bound %.4f" % (n, worst))


@pytest.mark.parametrize("n", [64, 65, 4097, 131074])
def test_gram_of_a_block_with_itself_is_exactly_symmetric(n):
    L = lib()
    rng = np.random.default_rng(7 * n)
    for m in (9, 24, 33):
        for ld in lds(n):
            store, _ = block(rng, n, m, ld)
            dV = buf(store)
            G = gram(L, n, m, dV, ld, m, dV, ld, m)[:m]
            assert np.all(np.isfinite(G))
            assert np.array_equal(G, G.T), (n, m, ld)


def test_gram_refuses_bad_arguments():
    L = lib()
    d = buf(np.zeros(64))
    assert L.psp_bv_gram(8, 2, d.ptr, 7, 2, d.ptr, 8, d.ptr, 2) != 0   # lda < n
    assert L.psp_bv_gram(8, 2, d.ptr, 8, 2, d.ptr, 8, d.ptr, 1) != 0   # ldg < ma
    assert L.psp_bv_gram(8, 2, None, 8, 2, d.ptr, 8, d.ptr, 2) != 0
    assert L.psp_bv_gram(-1, 2, d.ptr, 8, 2, d.ptr, 8, d.ptr, 2) != 0
    assert L.psp_bv_gram(8, 0, None, 8, 2, d.ptr, 8, None, 2) == 0     # nothing to do


def check_resid(n, k, ldax, ldmx, ldr, seed):
    L = lib()
    rng = np.random.default_rng(seed)
    sa, AX = block(rng, n, k, ldax)
    sm, MX = block(rng, n, k, ldmx)
    theta = rng.standard_normal(k) * 3.0
    slot = np.full(k, -1, dtype=np.int32)
    act = [c for c in range(k) if c % 3 != 1] if k > 1 else [0]
    for s, c in enumerate(act):
        slot[c] = s
    dA, dM, dth = buf(sa), buf(sm), buf(theta)
    dR, dn = buf(np.full((k, ldr), np.nan)), buf(np.full(k + 1, np.nan))
    assert L.psp_bv_resid(n, k, dA.ptr, ldax, dM.ptr, ldmx, dth.ptr, slot.ctypes.data, dR.ptr, ldr, dn.ptr) == 0, \
        L.psp_last_error()
    R = dR.download().reshape(k, ldr)
    nrm = dn.download()
    assert np.isnan(nrm[k])
    ref = AX - theta * MX  # the product rounded, then the difference
    for c in range(k):
        if slot[c] >= 0:
            assert np.array_equal(R[slot[c], :n], ref[:, c]), (n, k, c)
            assert np.all(np.isnan(R[slot[c], n:])), "padding rows written"
            col = C.c_void_p(dR.ptr + 8 * int(slot[c]) * ldr)
            h = tdot(L, n, 1, _Ptr(col), ldr, col)
            assert nrm[c] == h[0], (n, k, ldr, c)
        ext = float((ref[:, c].astype(LD) ** 2).sum())
        assert abs(nrm[c] - ext) <= 4 * np.sqrt(n) * EPS * ext
    assert np.all(np.isnan(R[len(act):])), "a column without a slot was written"
    dR2, dn2 = buf(np.full((k, ldr), np.nan)), buf(np.full(k + 1, np.nan))
    assert L.psp_bv_resid(n, k, dA.ptr, ldax, dM.ptr, ldmx, dth.ptr, slot.ctypes.data, dR2.ptr, ldr, dn2.ptr) == 0
    assert np.array_equal(R, dR2.download().reshape(k, ldr), equal_nan=True)
    assert np.array_equal(nrm, dn2.download(), equal_nan=True), "two runs differ"


class _Ptr(object):
    def __init__(self, ptr):
        self.ptr = ptr


@pytest.mark.parametrize("n", NS + FOLD_NS)
def test_resid(n):
    ks = (1, 4, 7, 32) if n <= 65539 else (5,)
    for k in ks:
        for ldax, ldmx, ldr in ((n, n, n), (n + 6, n + 6, n + 6), (n + 5, n + 6, n + 6), (n + 6, n + 6, n + 5),
                                (n + 5, n + 5, n + 5)):
            check_resid(n, k, ldax, ldmx, ldr, 31 * n + k)


def test_resid_refuses_bad_arguments():
    L = lib()
    d = buf(np.zeros(256))
    slot = np.arange(4, dtype=np.int32)
    ok = lambda *a: L.psp_bv_resid(*a)  # noqa: E731
    assert ok(8, 33, d.ptr, 8, d.ptr, 8, d.ptr, slot.ctypes.data, d.ptr, 8, d.ptr) != 0      # k beyond 32
    assert ok(8, 4, d.ptr, 7, d.ptr, 8, d.ptr, slot.ctypes.data, d.ptr, 8, d.ptr) != 0       # ldax < n
    bad = np.array([0, 1, 1, 2], dtype=np.int32)
    assert ok(8, 4, d.ptr, 8, d.ptr, 8, d.ptr, bad.ctypes.data, d.ptr, 8, d.ptr) != 0        # a slot given twice
    bad = np.array([0, 1, 4, 2], dtype=np.int32)
    assert ok(8, 4, d.ptr, 8, d.ptr, 8, d.ptr, bad.ctypes.data, d.ptr, 8, d.ptr) != 0        # a slot beyond k
    assert ok(8, 0, None, 8, None, 8, None, None, None, 8, None) == 0
