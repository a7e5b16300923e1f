"""GPU: the block product (psp_spmm.hip) and the batched PCG loop (psp_batch.hip) at the sizes where their kernels take the
branches that tests/test_gpu_spmm.py and tests/test_gpu_pcg_batch.py never reach.

Block products: csr_spmm_w4 places its workgroups of 512 rows in XCD stripes; below 8 * stripe workgroups (524 288 rows
for a csr_mat, 131 072 for the mirror of an sss_mat) the stripe round q / stripe is 0 for every workgroup.  The handles here
need two rounds (nine for the 3-D grid whose plane spans 128 workgroups); w4_stripe / w4_launch mirror the rule and
test_the_sizes_reach_the_stripe_rounds says so if a retuned stripe makes them stop doing that.  The bar is that of
test_gpu_spmm.py -- array_equal with matvec of the same handle, NaN padding and a spare column untouched, X only read, two
runs with equal bits -- and columns 0 and 8 are also array_equal with the CPU oracle's product, so that a block kernel that
is wrong together with its single-vector twin is caught as well.

Batched PCG: one case per loop psp_pcg can take for the single solve (batched PCG: "which loop a column is
compared with").  Each case asserts, after a single solve, which loop that was (last_solve_info), and then holds the batch
to the bar of test_gpu_pcg_batch.py: info and iter ==, relres equal as floats, x array_equal.  The brick loop is the one
exception the header of psp_batch.hip names: there the batch equals the launch-per-phase single solve bit for bit and
the brick loop within the bar test_gpu_brick.py uses between those two (relres 1e-6 relative, x 1e-12 * max|x|)."""
import functools

import numpy as np
import pytest

import test_gpu_pcg_batch as pb
import test_gpu_spmm as sm

pytestmark = pytest.mark.gpu

# the loops of psp_pcg that launch a kernel per phase (psp_solvers.hip: pcg_device_core)
LAUNCH_PER_PHASE = ("pcg_lazy", "pcg_lazy_pf", "pcg_eager", "pcg_host_scalars")


# ------------------------------------------------------------------------------------------------ block products

def w4_launch(n, stripe):
    """(workgroups that own rows, grid, stripe round of every workgroup that owns rows): w4_grid (psp_csr_tables.h) and the
    placement of csr_spmm_w4 / csr_spmv_w4"""
    wgs = -(-(-(-n // 128)) // 4)  # value blocks of 128 rows, four per workgroup
    grid = -(-wgs // (8 * stripe)) * (8 * stripe)
    rounds, seen = set(), set()
    for b in range(grid):
        q = b >> 3
        vb = ((q // stripe) * 8 + (b & 7)) * stripe + q % stripe
        assert 0 <= vb < grid and vb not in seen  # a permutation of the grid: every row block exactly once
        seen.add(vb)
        if vb < wgs:
            rounds.add(q // stripe)
    return wgs, grid, rounds


def w4_stripe(kind, grid):
    """w4_auto_stripe (psp_csr_select.h): 32 for the mirror of an sss_mat; an eighth of the plane (at least 16) when the
    farthest offset spans about 128 workgroups; 128 otherwise"""
    if kind == "sss":
        return 32
    nx, ny, nz = grid
    plane_wgs = (nx * ny if nz else nx) // 512
    if plane_wgs > 0 and 0.7 < 128.0 / plane_wgs < 1.5:
        s = 16
        while 2 * s <= plane_wgs // 8:
            s *= 2
        return s
    return 128


# name: (kind, grid, stripe rounds the handle must need)
BIG = {"csr725x724": ("csr", (725, 724, 0), 2), "big725x724": ("big", (725, 724, 0), 2),
       "released725x724": ("released", (725, 724, 0), 2), "csr256x256x9": ("csr", (256, 256, 9), 9),
       "sss363x362": ("sss", (363, 362, 0), 2)}
BIG_KS = (1, 3, 8, 9)  # KC = 1, 4, 8 and a second group of columns
BIG_KMAX = 9


def test_the_sizes_reach_the_stripe_rounds():
    for name, (kind, grid, want) in BIG.items():
        n = grid[0] * grid[1] * max(grid[2], 1)
        wgs, launched, rounds = w4_launch(n, w4_stripe(kind, grid))
        print(name, "n", n, "workgroups", wgs, "grid", launched, "rounds", sorted(rounds))
        assert rounds == set(range(want)) and want >= 2, name
    assert w4_launch(524900, 128)[:2] == (1026, 2048)  # two workgroups in round two
    assert w4_launch(589824, 16)[:2] == (1152, 1152) and w4_stripe("csr", (256, 256, 9)) == 16
    assert w4_launch(131406, 32)[:2] == (257, 512)
    # ... and no handle of test_gpu_spmm.py does: its largest matrix has 3 000 rows
    assert w4_launch(3000, 32)[2] == {0} and w4_launch(524288, 128)[2] == {0} and w4_launch(131072, 32)[2] == {0}


@functools.lru_cache(maxsize=None)
def oracle_matrix(kind, grid):
    from oracle import oracle as O
    return O.poisson_sss(*grid) if kind == "sss" else O.poisson_csr(*grid)


def big_handle(kind, grid):
    from pysparse_amd.device import DeviceCSR, DeviceSSS
    if kind == "sss":
        return DeviceSSS.poisson(*grid)
    if kind == "big":
        return DeviceCSR.poisson_big(*grid)
    A = DeviceCSR.poisson(*grid)
    if kind == "released":
        A.release_arrays()
    return A


@pytest.mark.parametrize("name", sorted(BIG))
def test_block_product_past_the_first_stripe_round(name):
    from pysparse_amd.device import DeviceBuffer
    kind, grid, _ = BIG[name]
    A = big_handle(kind, grid)
    n = A.shape[0]
    assert sm.kernel_name(A) == ("sss_spmv_w4" if kind == "sss" else "csr_spmv_w4")
    X = np.asfortranarray(np.random.default_rng(len(name)).standard_normal((n, BIG_KMAX)))
    ref = sm._reference(A, X, n)
    O = oracle_matrix("sss" if kind == "sss" else "csr", grid)
    for c in (0, BIG_KMAX - 1):  # the independent reference
        y = np.empty(n)
        O.matvec(np.ascontiguousarray(X[:, c]), y)
        assert np.array_equal(ref[:, c], y), (name, c)
    for pad in (5, 6):  # n is even: an odd and an even leading dimension
        ld = n + pad
        Xb = np.full((ld, BIG_KMAX + 1), np.nan, order="F")
        Xb[:n, :BIG_KMAX] = X
        nan_block = np.full(ld * (BIG_KMAX + 1), np.nan)
        dx = DeviceBuffer.from_host(Xb.ravel(order="F"))  # X goes up once per leading dimension
        dy = DeviceBuffer(ld * (BIG_KMAX + 1))
        first = None
        for k in BIG_KS + ((BIG_KMAX,) if pad == 5 else ()):  # pad 5: k = 9 twice
            dy.upload(nan_block)
            A.matmat_dev(k, dx.ptr, ld, dy.ptr, ld)
            sm._lib().psp_synchronize()
            out = dy.download().reshape((ld, BIG_KMAX + 1), order="F")
            assert np.array_equal(out[:n, :k], ref[:, :k]), (name, k, pad)
            assert np.isnan(out[n:, :]).all() and np.isnan(out[:, k:]).all(), (name, k, pad)
            if k == BIG_KMAX:
                if first is None:
                    first = out
                else:
                    assert np.array_equal(first, out, equal_nan=True), (name, pad)
        assert np.array_equal(dx.download().reshape((ld, BIG_KMAX + 1), order="F"), Xb, equal_nan=True)  # X is only read
        dx.free()
        dy.free()


# ------------------------------------------------------------------------------------------------ batched PCG

def single_loop(S, K, kname, maxit, c=1):
    """the loop psp_pcg takes for column c of S alone (column 1: a random right-hand side, x0 = 0)"""
    from pysparse_amd.device import last_solve_info
    assert (c, maxit, kname) not in S.single
    S.solve_alone(c, maxit, K, kname)
    name, d = last_solve_info()
    print(kname, "n", S.n, "maxit", maxit, "single solve:", name, d)
    return name, d


def precon(kname, S):
    from pysparse_amd.device import DeviceJacobi
    return DeviceJacobi(S.A, 1.0, 1) if kname.startswith("jacobi1") else None


class switched_off:
    """set_single_kernel_loops(False) for the block, True again behind it"""

    def __enter__(self):
        from pysparse_amd.device import set_single_kernel_loops
        set_single_kernel_loops(False)

    def __exit__(self, *exc):
        from pysparse_amd.device import set_single_kernel_loops
        set_single_kernel_loops(True)
        return False


def spans(n):
    return -(-n // 512)


@functools.lru_cache(maxsize=None)
def mid_system(form):
    from pysparse_amd.device import DeviceCSR, DeviceSSS
    A = (DeviceCSR if form == "csr" else DeviceSSS).poisson(182, 181)
    return pb.System(A, 182 * 181, pb.smooth_column(182, 181), 11)


@pytest.mark.parametrize("form", ["csr", "sss"])
@pytest.mark.parametrize("kname", ["none", "jacobi1"])
def test_batch_equals_the_mid_size_single_kernel_loop(form, kname):
    S = mid_system(form)
    assert S.n == 32942 and S.n >= 1 << 15
    K = precon(kname, S)
    for maxit in (2000, 7):
        assert single_loop(S, K, kname, maxit)[0] == "pcg_mid"
        for k in (3, 9):
            info, it = pb.check_batch(S, K, kname, k, 5, maxit)
            if maxit == 7:
                assert info[1] == -1 and it[1] == 8
            else:
                assert info[0] == 0 and info[1] == 0
            if k == 9:
                assert info[2] == 0 and it[2] == 0 and info[3] == 0 and it[3] == 0
                assert info[4] == 0 and (maxit == 7 or it[4] < it[5])


def test_more_than_256_spans_two_groups_in_the_finish():
    from pysparse_amd.device import DeviceCSR
    n = 363 * 362
    assert spans(n) == 257  # kTailGroup + 1: reduce_block(raw) with two groups, three values per column
    S = pb.System(DeviceCSR.poisson(363, 362), n, pb.smooth_column(363, 362), 12)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        assert single_loop(S, K, kname, 25)[0] == "pcg_mid"
        for k in (3, 9):
            info, it = pb.check_batch(S, K, kname, k, 5, 25)
            assert info[1] == -1 and it[1] == 26


def varying_2d(nx, ny, seed):
    """5-point operator with random symmetric couplings and a dominant, varying diagonal"""
    import scipy.sparse as sp
    n = nx * ny
    g = np.random.default_rng(seed)
    i = np.arange(n) % nx
    e1 = -(0.1 + g.random(n - 1)) * (i[:-1] < nx - 1)
    e2 = -(0.1 + g.random(n - nx))
    M = sp.diags([e2, e1, e1, e2], [-nx, -1, 1, nx], shape=(n, n), format="csr")
    M = (M + sp.diags(-np.asarray(M.sum(axis=1)).ravel() + 0.05 + g.random(n))).tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    return M


def test_varying_coefficients_beyond_the_mid_size_loop():
    from pysparse_amd.device import DeviceCSR
    nx, ny = 1100, 1000
    n = nx * ny
    assert spans(n) == 2149
    M = varying_2d(nx, ny, 13)
    A = DeviceCSR.from_arrays(M.shape, M.indptr, M.indices, M.data)
    assert sm.kernel_name(A) == "csr_spmv_w4"
    S = pb.System(A, n, None, 14, ncols=3)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        name, d = single_loop(S, K, kname, 12)
        # 2^20 < n <= 2^21 with varying coefficients: psp_mid.hip declines, no grid for the bricks, too large for
        # psp_coop.hip, below the 2^21 rows of the folded product -- the lazy launch-per-phase loop
        assert name == "pcg_lazy"
        assert d["dinv_streamed"] == (kname == "jacobi1")
        info, it = pb.check_batch(S, K, kname, 3, 5, 12)
        assert info[1] == -1 and it[1] == 13 and info[2] == 0 and it[2] == 0


def test_beyond_4096_spans_and_the_folded_product(oracle):
    from pysparse_amd.device import DeviceCSR, pcg_batch
    n = 1449 * 1449
    assert n > 1 << 21 and spans(n) == 4101  # 17 groups: group_fold_kernel + finish in the single solve
    A = DeviceCSR.poisson(1449, 1449)
    S = pb.System(A, n, None, 15, ncols=2)
    O = oracle.poisson_csr(1449, 1449)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        assert single_loop(S, K, kname, 12)[0] == "pcg_lazy_pf"
        X = np.asfortranarray(S.X0[:, :2].copy())
        B = np.asfortranarray(S.B[:, :2])
        info, it, rr = pcg_batch(A, B, X, pb.TOL, 12, K)
        for c in range(2):
            (i1, it1, rr1), x1 = S.solve_alone(c, 12, K, kname)
            print(kname, "col", c, "batch", (info[c], it[c], rr[c]), "alone", (i1, it1, rr1))
            assert (info[c], it[c]) == (i1, it1) == (-1, 13)
            assert float(rr[c]) == float(rr1)
            assert np.array_equal(X[:, c], x1)
            # the independent reference: the true residual of the returned x, formed on the host with the oracle's product
            y = np.empty(n)
            O.matvec(np.ascontiguousarray(X[:, c]), y)
            true = np.linalg.norm(B[:, c] - y) / np.linalg.norm(B[:, c])
            print(kname, "col", c, "true relres", true, "returned", rr[c])
            assert abs(true - rr[c]) <= 1e-6 * true


def test_brick_loop_both_halves():
    """psp_batch.hip: a column "agrees with the brick loop to rounding only" -- it IS the launch-per-phase single solve,
    whatever the switch says, and meets the brick loop within the bar of test_gpu_brick.py"""
    from pysparse_amd.device import DeviceCSR, pcg_batch
    n = 50 * 54 * 60
    S = pb.System(DeviceCSR.poisson(50, 54, 60), n, None, 16, ncols=3)
    k = 3
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        for maxit in (2000, 7):
            assert single_loop(S, K, kname, maxit)[0] == "pcg_brick"
            with switched_off():
                assert single_loop(S, K, kname + "/off", maxit)[0] in LAUNCH_PER_PHASE
                pb.check_batch(S, K, kname + "/off", k, 5, maxit)  # batch == single, bit for bit
            X = np.asfortranarray(S.X0[:, :k].copy())
            info, it, rr = pcg_batch(S.A, np.asfortranarray(S.B[:, :k]), X, pb.TOL, maxit, K)  # the switch is on again
            for c in range(k):
                (i0, it0, rr0), x0 = S.solve_alone(c, maxit, K, kname + "/off")
                assert (info[c], it[c]) == (i0, it0) and float(rr[c]) == float(rr0) and np.array_equal(X[:, c], x0), c
                (i1, it1, rr1), x1 = S.solve_alone(c, maxit, K, kname)  # the brick loop
                print(kname, maxit, "col", c, "batch", (info[c], it[c], rr[c]), "brick", (i1, it1, rr1))
                assert (info[c], it[c]) == (i1, it1), c
                assert abs(rr[c] - rr1) <= 1e-6 * rr1, c
                assert np.abs(X[:, c] - x1).max() <= 1e-12 * np.abs(x1).max(), c
            assert info[2] == 0 and it[2] == 0
            assert (info[1], it[1]) == ((-1, 8) if maxit == 7 else (0, it[1]))


@pytest.mark.parametrize("sysname", ["csr33x31", "csr100x100", "sss33x31"])
def test_switch_off_small_systems(sysname):
    S = pb.system(sysname)
    for kname in ("none", "jacobi1"):
        K = pb.make_precon(kname, S)
        assert single_loop(S, K, kname + "/on", 2000)[0] == "pcg_coop"  # (a key of its own: solved whatever ran before)
        with switched_off():
            assert single_loop(S, K, kname + "/off", 2000)[0] in LAUNCH_PER_PHASE
            for k in (3, 9):
                info, it = pb.check_batch(S, K, kname + "/off", k, 5, 2000)
                assert info[0] == 0 and info[1] == 0
                if k == 9:
                    assert info[2] == 0 and it[2] == 0 and info[3] == 0 and it[3] == 0 and it[4] < it[5]


def irregular_short_rows(n, seed):
    """irregular SPD matrix: at most 3 random couplings drawn per row, made symmetric, a coupling dropped where it would
    give either of its rows more than 8 entries (diagonal included), strongly dominant diagonal"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), 3)
    c = rng.integers(0, n, size=r.size)
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    pairs = np.unique(np.stack([lo, hi], axis=1)[lo != hi], axis=0)
    pairs = pairs[rng.permutation(len(pairs))]
    deg = np.zeros(n, dtype=np.int64)
    keep = np.zeros(len(pairs), dtype=bool)
    for e, (a, b) in enumerate(pairs.tolist()):
        if deg[a] < 7 and deg[b] < 7:
            deg[a] += 1
            deg[b] += 1
            keep[e] = True
    pairs = pairs[keep]
    v = -rng.uniform(0.1, 1.0, size=len(pairs))
    M = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([pairs[:, 0], pairs[:, 1]]),
                                                np.concatenate([pairs[:, 1], pairs[:, 0]]))), shape=(n, n)).tocsr()
    M = (M + sp.diags(2.0 * np.asarray(abs(M).sum(axis=1)).ravel() + rng.uniform(0.5, 1.0, size=n))).tocsr()
    M.sort_indices()
    assert np.diff(M.indptr).max() <= 8 and (deg == 7).any()
    return M


@pytest.mark.parametrize("n", [3000, 40000])
def test_coop_order_for_a_general_matrix(n):
    """rows of at most 8 entries and no index-free layout: csr_spmm_rows, then p.q as a dot of its own in the order of
    psp_coop.hip (3 and 40 workgroups of 1024 rows)"""
    from pysparse_amd.device import DeviceCSR
    M = irregular_short_rows(n, 17)
    A = DeviceCSR.from_arrays(M.shape, M.indptr, M.indices, M.data)
    assert sm.kernel_name(A) != "csr_spmv_w4"  # not index-free
    S = pb.System(A, n, None, 18)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        for maxit in (2000, 5):
            assert single_loop(S, K, kname, maxit)[0] == "pcg_coop"
            for k in (3, 9):
                info, it = pb.check_batch(S, K, kname, k, 5, maxit)
                assert (info[1], it[1]) == ((-1, 6) if maxit == 5 else (0, it[1]))
    assert A.setup_info()["reorder_state"] != 1 and A.setup_info()["products_counted"] < 2048


@pytest.mark.parametrize("how", ["poisson_big", "released"])
def test_index_free_only_handles_are_not_in_coop_order(how):
    from pysparse_amd.device import DeviceCSR
    if how == "poisson_big":
        A = DeviceCSR.poisson_big(33, 31)
    else:
        A = DeviceCSR.poisson(33, 31)
        A.release_arrays()
    assert sm.kernel_name(A) == "csr_spmv_w4"
    S = pb.System(A, 33 * 31, pb.smooth_column(33, 31), 19)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        name = single_loop(S, K, kname, 2000)[0]
        assert name != "pcg_coop" and name in LAUNCH_PER_PHASE  # the plain handle of this size is pcg_coop
        for k in (3, 9):
            info, it = pb.check_batch(S, K, kname, k, 5, 2000)
            assert info[0] == 0 and info[1] == 0
            if k == 9:
                assert info[2] == 0 and it[2] == 0 and info[3] == 0 and it[3] == 0 and it[4] < it[5]


def band_spd(n, half, per_row, seed):
    """random symmetric band matrix, far more distinct offsets than an index-free layout takes, SPD by dominance"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = r + rng.integers(1, half + 1, size=r.size)
    ok = c < n
    U = sp.coo_matrix((-rng.uniform(0.1, 1.0, size=int(ok.sum())), (r[ok], c[ok])), shape=(n, n)).tocsr()  # duplicates add
    M = (U + U.T).tocsr()
    M = (M + sp.diags(2.0 * np.asarray(abs(M).sum(axis=1)).ravel() + rng.uniform(0.5, 1.0, size=n))).tocsr()
    M.sort_indices()
    return M


def test_another_kernel_family_with_many_partial_sums():
    """a product that is not csr_spmv_w4: the batch multiplies column by column with the single product, whose fused dot
    leaves one partial sum per workgroup in w->partials (stride kMaxParts), added by a k = 1 finish of 1 024 threads"""
    from pysparse_amd.device import DeviceCSR
    n = 150000
    M = band_spd(n, 150, 6, 20)
    offsets = np.unique(M.indices - np.repeat(np.arange(n), np.diff(M.indptr)))
    assert len(offsets) > 64
    A = DeviceCSR.from_arrays(M.shape, M.indptr, M.indices, M.data)
    kn, kinfo = A.kernel_info()
    print("band matrix: nnz", M.nnz, "kernel", kn, kinfo)
    # csr_spmv_w3: a workgroup of four waves, one chunk of at most 1 024 stored entries per wave (get_chunk_table,
    # csr_spmv_launch), one partial sum per workgroup -- so at least nnz / 4096 of them
    assert kn == "csr_spmv_w3"
    assert -(-(-(-M.nnz // 1024)) // 4) > 256
    S = pb.System(A, n, None, 21, ncols=3)
    for kname in ("none", "jacobi1"):
        K = precon(kname, S)
        assert single_loop(S, K, kname, 2000)[0] in LAUNCH_PER_PHASE
        info, it = pb.check_batch(S, K, kname, 3, 5, 2000)
        assert info[0] == 0 and info[1] == 0 and info[2] == 0 and it[2] == 0 and it[1] > 3
    si = A.setup_info()
    assert si["reorder_state"] != 1 and si["products_counted"] < 2048
    assert sm.kernel_name(A) == "csr_spmv_w3"
