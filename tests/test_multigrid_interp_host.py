"""CPU: precon.multigrid(..., galerkin=True, interp='operator') / device.DeviceMultigridInterp -- the keyword and its checks
before any device call, the new C symbols, and the oracle of the Galerkin V-cycle with operator-dependent interpolation
(DESIGN.md section 9j): the weights of every level from the level operator's own stencil, P, R = P' / 2^(coarsened axes),
A_{l+1} = R A_l P, the cycle in float64 and the same cycle in np.longdouble.  tests/test_gpu_multigrid_interp.py imports the
oracle and the operator generators from here.  Nothing here needs a GPU.

The tests under "the feature" exercise the library and fail without it.  The tests under "oracle guards" guard the
yardstick, not the code.

The test operators are -div(kappa grad u) + s u, cell-centred with harmonic face averages and Dirichlet ends (the assembly
of tests/test_multigrid_galerkin_host.varying_operator), with kappa = 1 but for random blocks of b cells a side that hold
`hi`, each block drawn with probability `frac`; and, for stencil='box', the Q1 form of tests/test_multigrid_box_host with
such a kappa per element."""
import functools
import inspect
import itertools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from test_multigrid_host import level_grids
from test_multigrid_galerkin_host import GalerkinOracle, _LdMat, varying_operator
from test_multigrid_box_host import pcg_margin, q1kappa_operator

LD = np.longdouble
EPS = np.finfo(np.float64).eps

# ------------------------------------------------------------------------------------------------ the test operators


def block_kappa(shape, block, hi, frac, seed):
    """1, and `hi` in the blocks of `block` cells a side drawn with probability `frac`; shape as numpy indexes it"""
    rng = np.random.default_rng([seed, block, len(shape)] + list(shape))
    coarse = rng.random(tuple(-(-m // block) for m in shape)) < frac
    k = coarse
    for ax in range(len(shape)):
        k = np.repeat(k, block, axis=ax)
    k = k[tuple(slice(0, m) for m in shape)]
    return np.where(k, float(hi), 1.0)


def kappa_operator(grid, kap, s=0.0):
    """varying_operator's assembly for a given cell field kap of shape grid[::-1]"""
    grid = tuple(int(g) for g in grid)
    nd, n = len(grid), int(np.prod(grid))
    idx = np.arange(n).reshape(kap.shape)
    diag = np.full(kap.shape, float(s))
    rows, cols, vals = [], [], []
    for a, m in enumerate(grid):
        ax = nd - 1 - a
        if m == 1:
            continue
        lo = [slice(None)] * nd
        hi = [slice(None)] * nd
        lo[ax], hi[ax] = slice(0, m - 1), slice(1, m)
        lo, hi = tuple(lo), tuple(hi)
        h = 2.0 * kap[lo] * kap[hi] / (kap[lo] + kap[hi])
        low, up = kap.copy(), kap.copy()
        low[hi] = h
        up[lo] = h
        diag = diag + low + up
        rows += [idx[lo].ravel(), idx[hi].ravel()]
        cols += [idx[hi].ravel(), idx[lo].ravel()]
        vals += [-h.ravel(), -h.ravel()]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


# name -> (block, hi, frac); 'single' is the case the feature does not cure
BLOCKS = {"b8_1e4": (8, 1.0e4, 0.3), "b5_1e6": (5, 1.0e6, 0.4), "b4_1e4": (4, 1.0e4, 0.3), "b3_1e6": (3, 1.0e6, 0.4),
          "b3_1e4": (3, 1.0e4, 0.3),          "b2_1e4": (2, 1.0e4, 0.3), "single": (1, 1.0e4, 0.3)}


def interp_operator(grid, kind, s=0.0, seed=0):
    """kind: a name of BLOCKS, 'const', 'smooth' (section 9d's), or 'box_' + a name of BLOCKS: the Q1 form with kappa per
    element (the full pattern, for stencil='box')"""
    grid = tuple(int(g) for g in grid)
    if kind in ("const", "smooth"):
        return varying_operator(grid, kind, s, seed)
    if kind.startswith("box_"):
        b, hi, frac = BLOCKS[kind[4:]]
        return q1kappa_operator(grid, kappa=block_kappa(tuple(g + 1 for g in grid)[::-1], b, hi, frac, seed))
    b, hi, frac = BLOCKS[kind]
    return kappa_operator(grid, block_kappa(grid[::-1], b, hi, frac, seed), s)


# ------------------------------------------------------------------------------------------------ the oracle

def stencil_arrays(grid, rows, cols, vals):
    """S[d0 + 1, d1 + 1, .., p] = A[p, p + d] for the entries given as triples; absent entries 0"""
    nd, N = len(grid), int(np.prod(grid))
    st = np.cumprod((1,) + tuple(grid[:-1]))
    S = np.zeros((3,) * nd + (N,), dtype=vals.dtype)
    d = [(cols // st[a]) % grid[a] - (rows // st[a]) % grid[a] for a in range(nd)]
    assert all(np.abs(x).max() <= 1 for x in d)
    S[tuple(x + 1 for x in d) + (rows,)] = vals
    return S


def operator_weights(grid, rows, cols, vals, c_eps=0.0):
    """Section 9j's weights of the level with grid `grid` and the operator given as triples, in the triples' dtype:
    (W[slot, p], the points that took the linear weights, the smallest decision margin |T0| / sum |T| over the points whose
    T are not all 0, E[slot, p]).  E is the bound c_eps * sum |T[delta] / T0| |w_{p + delta}| accumulated through the
    rounds: E_p = sum |T[delta] / T0| (c_eps |w_{p + delta}| + E_{p + delta}).
    Slot bit a: 0 the lower (or only) parent along axis a, 1 the upper one.  The sums run in the order of the kernels: the
    collapse over d in ascending number (d0 fastest), the accumulation over delta in ascending number."""
    grid = tuple(int(g) for g in grid)
    nd, N, dt = len(grid), int(np.prod(grid)), vals.dtype
    st = np.cumprod((1,) + grid[:-1])
    co = [m >= 4 for m in grid]
    S = stencil_arrays(grid, rows, cols, vals)
    p = np.arange(N)
    c = [(p // st[a]) % grid[a] for a in range(nd)]
    between = [np.full(N, co[a]) & (c[a] % 2 == 0) for a in range(nd)]
    W = np.zeros((2 ** nd, N), dtype=dt)
    E = np.zeros((2 ** nd, N), dtype=dt)
    m0 = ~np.any(between, axis=0)
    W[0, m0] = 1
    fallbacks, margin = 0, np.inf
    codes = [d[::-1] for d in itertools.product((-1, 0, 1), repeat=nd)]  # ascending number: d0 fastest
    for rnd in range(1, nd + 1):
        for F in itertools.combinations(range(nd), rnd):
            sel = np.ones(N, dtype=bool)
            for a in range(nd):
                sel &= between[a] == (a in F)
            pts = p[sel]
            if pts.size == 0:
                continue
            T = {}
            for t in codes:
                if any(t[a] != 0 and a not in F for a in range(nd)):
                    continue
                acc = np.zeros(pts.size, dtype=dt)
                for d in codes:
                    if all(d[a] == t[a] for a in F):
                        acc = acc + S[tuple(x + 1 for x in d)][pts]
                T[t] = acc
            T0 = T[(0,) * nd]
            fine = np.isfinite(T0) & (T0 > 0)
            tot = sum(np.abs(v) for v in T.values())
            live = tot > 0
            if live.any():
                margin = min(margin, float((np.abs(T0[live]) / tot[live]).min()))
            fallbacks += int((~fine).sum())
            T0s = np.where(fine, T0, 1)
            for s in range(2 ** nd):
                if any((s >> a) & 1 and a not in F for a in range(nd)):
                    continue
                acc = np.zeros(pts.size, dtype=dt)
                lin = np.zeros(pts.size, dtype=dt)
                err = np.zeros(pts.size, dtype=dt)
                for t in codes:
                    if t not in T or not any(t):
                        continue
                    if any(t[a] != 0 and (t[a] > 0) != bool((s >> a) & 1) for a in range(nd)):
                        continue
                    inside = np.ones(pts.size, dtype=bool)
                    for a in range(nd):
                        inside &= (c[a][pts] + t[a] >= 0) & (c[a][pts] + t[a] < grid[a])
                    sq = sum(((s >> a) & 1) << a for a in range(nd) if t[a] == 0)
                    q = np.where(inside, pts + sum(t[a] * st[a] for a in range(nd)), 0)
                    wq = np.where(inside, W[sq, q], 0)
                    coef = T[t] / T0s
                    acc = acc + coef * wq
                    err = err + np.abs(coef) * (c_eps * np.abs(wq) + np.where(inside, E[sq, q], 0))
                    if all(t[a] != 0 for a in F):
                        lin = lin + wq
                W[s, pts] = np.where(fine, 0 - acc, lin * dt.type(0.5) ** rnd)
                E[s, pts] = np.where(fine, err, 0)
    return W, fallbacks, margin, E


def prolongation(grid, W):
    """(indptr, indices, data) of P in CSR from the weights: the row of a fine point holds its slots in ascending number,
    those whose parent exists"""
    grid = tuple(int(g) for g in grid)
    nd, N = len(grid), int(np.prod(grid))
    st = np.cumprod((1,) + grid[:-1])
    co = [m >= 4 for m in grid]
    nc = [m // 2 if k else m for m, k in zip(grid, co)]
    stc = np.cumprod((1,) + tuple(nc[:-1]))
    p = np.arange(N)
    c = [(p // st[a]) % grid[a] for a in range(nd)]
    rows, cols, vals = [], [], []
    for s in range(2 ** nd):
        ok = np.ones(N, dtype=bool)
        col = np.zeros(N, dtype=np.int64)
        for a in range(nd):
            up = (s >> a) & 1
            if not co[a]:
                j = c[a]
                ok &= not up
            else:
                even = c[a] % 2 == 0
                j = np.where(even, c[a] // 2 - 1 + up, (c[a] - 1) // 2)
                ok &= even | (not up)
            ok &= (j >= 0) & (j < nc[a])
            col += j * stc[a]
        rows.append(p[ok])
        cols.append(col[ok])
        vals.append(W[s, ok])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order], (N, int(np.prod(nc)))


def _ld_rap(A, Prows, Pcols, Pvals, shape, scale):
    """P' A P * scale in longdouble with P given as sorted triples: every product as a triple, one sum per (K, J)"""
    nf, nc = shape
    ptr = np.concatenate([[0], np.cumsum(np.bincount(Prows, minlength=nf))])

    def expand(keep, along, vals):
        cnt = ptr[along + 1] - ptr[along]
        rep = np.repeat(np.arange(along.size), cnt)
        pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(ptr[along], cnt)
        return keep[rep], Pcols[pos], vals[rep] * Pvals[pos]

    i, J, v = expand(A.rows, A.cols, A.vals)
    J2, K, v = expand(J, i, v)
    v = v * LD(scale)
    key = K.astype(np.int64) * nc + J2
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    ukey, starts = np.unique(key, return_index=True)
    return _LdMat(ukey // nc, ukey % nc, np.add.reduceat(v, starts), (nc, nc))


class InterpOracle(GalerkinOracle):
    """GalerkinOracle with section 9j's P: per level the weights from the level's own operator, in float64 from the float64
    chain and in np.longdouble from the longdouble chain; apply / apply_ext are the parent's.  W[l], fallbacks[l] and
    margin[l] are the float64 leg's; fallbacks_ext[l] the longdouble leg's."""

    def __init__(self, grid, A):
        assert np.finfo(LD).eps < 1e-18, "np.longdouble is not an extended format here: the yardstick is missing"
        self.grids = level_grids(grid)
        A = A.tocsr()
        A.sort_indices()
        self.A, self.P, self.R = [A], [], []
        self.Ax, self.Px, self.Rx = [_LdMat.from_scipy(A)], [], []
        self.W, self.fallbacks, self.margin, self.fallbacks_ext = [], [], [], []
        for g in self.grids[:-1]:
            co = [m >= 4 for m in g]
            scale = 1.0 / 2.0 ** sum(co)
            C = self.A[-1].tocoo()
            W, fb, mg, _ = operator_weights(g, C.row, C.col, C.data)
            r, c, v, shape = prolongation(g, W)
            P = sp.csr_matrix((v, (r, c)), shape=shape)
            R = (P.T * scale).tocsr()
            self.W.append(W)
            self.fallbacks.append(fb)
            self.margin.append(mg)
            self.P.append(P)
            self.R.append(R)
            Ac = (R @ self.A[-1] @ P).tocsr()
            Ac.sort_indices()
            self.A.append(Ac)
            Ax = self.Ax[-1]
            Wx, fbx, _, _ = operator_weights(g, Ax.rows, Ax.cols, Ax.vals)
            rx, cx, vx, _ = prolongation(g, Wx)
            self.fallbacks_ext.append(fbx)
            self.Px.append(_LdMat(rx, cx, vx, shape))
            order = np.lexsort((rx, cx))
            self.Rx.append(_LdMat(cx[order], rx[order], vx[order] * LD(scale), shape[::-1]))
            self.Ax.append(_ld_rap(Ax, rx, cx, vx, shape, scale))
        self.d = [M.diagonal() for M in self.A]
        self.dx = []
        for M in self.Ax:
            m = M.rows == M.cols
            d = np.zeros(M.shape[0], dtype=LD)
            d[M.rows[m]] = M.vals[m]
            self.dx.append(d)
        self.inv = np.linalg.inv(self.A[-1].toarray())
        Ad = self.Ax[-1].toarray()
        X = self.inv.astype(LD)
        two = 2.0 * np.eye(Ad.shape[0], dtype=LD)
        for _ in range(2):  # Newton: X <- X (2 I - A X)
            X = X @ (two - Ad @ X)
        self.invx = X


@functools.lru_cache(maxsize=None)
def interp_oracle_for(grid, kind, s=0.0, seed=0):
    grid = tuple(grid)
    return InterpOracle(grid, interp_operator(grid, kind, s, seed))


@functools.lru_cache(maxsize=None)
def linear_oracle_for(grid, kind, s=0.0, seed=0):
    grid = tuple(grid)
    return GalerkinOracle(grid, interp_operator(grid, kind, s, seed))


def rhs(grid, seed=0):
    return np.random.default_rng(seed).random(int(np.prod(grid)))


# The operators of the GPU comparisons: (grid, kind, s, seed).  Every one satisfies the decision margin below.
GPU_CASES = [
    ((7,), "b2_1e4", 0.0, 0), ((64,), "b5_1e6", 0.0, 0), ((9, 7), "b2_1e4", 0.0, 0), ((13, 11), "b3_1e6", 0.0, 0),
    ((40, 5), "b4_1e4", 0.0, 0), ((70, 45), "b5_1e6", 0.0, 0), ((64, 64), "b8_1e4", 0.0, 0), ((64, 64), "smooth", 0.0, 0),
    ((13, 11), "box_b3_1e6", 0.0, 0), ((64, 64), "box_b8_1e4", 0.0, 0),
    ((6, 7, 9), "b2_1e4", 0.0, 0), ((9, 7, 6), "b3_1e6", 0.0, 0), ((8, 8, 8), "const", 0.3, 0), ((9, 7, 6), "box_b2_1e4", 0.0, 0),
    ((26, 37, 21), "b3_1e6", 0.0, 0), ((32, 32, 32), "b4_1e4", 0.0, 1),
]

# PCG to 1e-8 from x = 0 on b = rhs(grid, seed), omega 0.8, 2 steps: (kind, grid) -> (seed, iterations with the oracle's
# float64 cycle with operator-dependent interpolation, with section 9d's linear one, with Jacobi), measured by
# test_the_table_is_what_the_oracle_gives.  The seeds are the first from 3 on for which the recurrence residual of the
# operator-dependent solve at its last iteration and at the one before is more than 10 % away from tol ||b||.
PCG_TABLE = {
    ("b8_1e4", (64, 64)): (3, 12, 39, 544),
    ("b8_1e4", (128, 128)): (3, 20, 63, 2267),
    ("b5_1e6", (64, 64)): (3, 19, 94, 1334),
    ("b5_1e6", (128, 128)): (3, 52, 144, 3001),  # Jacobi: not converged in 3000
    ("b5_1e6", (70, 45)): (3, 21, 54, 702),
    ("b4_1e4", (32, 32, 32)): (3, 23, 74, 940),  # kappa of seed 1 (OP_SEED): with seed 0 every right-hand side stops within 5 %
    ("b3_1e6", (26, 37, 21)): (3, 34, 102, 827),
    ("box_b8_1e4", (64, 64)): (3, 9, 18, 296),
    ("smooth", (64, 64)): (3, 8, 7, 208),
    ("single", (64, 64)): (3, 79, 197, 1898),  # single cells: the case the feature does not cure
}


# the seed of kappa where it is not 0
OP_SEED = {("b4_1e4", (32, 32, 32)): 1}

# Rows whose count the reference itself does not pin down.  With blocks of 1e6 the matrices have condition numbers of 1e8
# and more (3.4e8 at 64^2): cond * eps is the tolerance 1e-8 itself, and NumPy PCG with the oracle's cycle is then sensitive
# to its own roundings.  Three variations of the oracle's solve are tried, none of which changes the algorithm: the cycle
# evaluated in np.longdouble (on rows of at most 16384 points and 60 iterations), and the dot products of the PCG loop
# summed in another order (reversed, in np.longdouble, and under two seeded permutations).  At 64^2 the counts are 19 and 20
# and the TRUE residual of the float64 solve is 1.004e-8 ||b||; at 128^2 52 to 59 with true residuals of 1.1e-7 ||b||; at
# (26, 37, 21) one permutation of the dot products stops after 33 iterations instead of 34, and the residual of the
# iteration before the stop ranges from 1.06 to 4.34 tol ||b|| over the variations -- the 10 % rule for seeds does not
# protect a count there.  A further rounding of the same algorithm -- the device's -- cannot be held to "exactly the
# oracle's iterations with true residual <= 1e-8" on such a row.  test_unstable_rows_are_unstable_in_the_oracle_itself
# asserts that a row is listed here iff the oracle's variations disagree or its true residual misses 1e-8, and records what
# the oracle does pin down: the range of its counts and its worst true residual.  The GPU test asserts on these rows a count
# inside that range and a true residual of at most twice that worst one (a further rounding of the same algorithm may be
# as far from the variations as they are from each other, not further).  Every other
# row, the 1e6 row (70, 45) included, gives one count under all variations and is asserted exactly.
# -> (the smallest and the largest count over the variations, the worst true residual over them in ||b||)
UNSTABLE = {("b5_1e6", (64, 64)): (19, 20, 1.4e-8), ("b5_1e6", (128, 128)): (52, 59, 1.25e-7),
            ("b3_1e6", (26, 37, 21)): (33, 34, 6.5e-9)}


def _dot_variant(v):
    if v == 0:
        return lambda a, b: a @ b
    if v == 1:
        return lambda a, b: (a[::-1] * b[::-1]).sum()
    if v == 2:
        return lambda a, b: float(np.sum((a * b).astype(LD)))
    return lambda a, b: np.add.reduce((a * b).reshape(-1, 1)[np.random.default_rng(v).permutation(a.size), 0])


def oracle_pcg_variant(A, b, tol, maxit, precon, v):
    """oracle_pcg with the dot products of variation v"""
    dot = _dot_variant(v)
    x = np.zeros_like(b)
    r = b.copy()
    tolb = tol * np.sqrt(dot(b, b))
    rho, p = 1.0, None
    for it in range(1, maxit + 1):
        z = precon(r)
        rho1, rho = rho, dot(r, z)
        p = z if it == 1 else z + (rho / rho1) * p
        q = A @ p
        alpha = rho / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        if np.sqrt(dot(r, r)) <= tolb:
            return it, x
    return maxit + 1, x


def oracle_pcg(A, b, tol, maxit, precon):
    """the loop of pcg_margin, returning (iterations, x)"""
    x = np.zeros_like(b)
    r = b.copy()
    tolb = tol * np.linalg.norm(b)
    rho, p = 1.0, None
    for it in range(1, maxit + 1):
        z = precon(r)
        rho1, rho = rho, r @ z
        p = z if it == 1 else z + (rho / rho1) * p
        q = A @ p
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        if np.linalg.norm(r) <= tolb:
            return it, x
    return maxit + 1, x


# ------------------------------------------------------------------------------------------------ the feature

def ll(n, m=None):
    from pysparse.sparse import spmatrix
    A = spmatrix.ll_mat(n, m or n)
    for i in range(min(n, m or n)):
        A[i, i] = 2.0
    return A


def fake_csr(shape):
    from pysparse_amd import device

    class FakeCSR(device.DeviceCSR):
        def __init__(self, shape):  # no handle: nothing may reach the library
            self._h = None
            self.shape = shape

    return FakeCSR(shape)


def test_interp_is_a_keyword_and_documented():
    from pysparse.precon import precon
    assert "interp='linear'" in precon.multigrid.__doc__ and "'operator'" in precon.multigrid.__doc__
    with pytest.raises(TypeError):  # not a positional argument
        precon.multigrid(ll(6), (6,), 0.8, 2, True, "double", None, "axis", "operator")


@pytest.mark.parametrize("bad", [1, None, b"operator", True, ("operator",)], ids=["int", "None", "bytes", "bool", "tuple"])
def test_an_interp_that_is_no_str_is_a_type_error(bad):
    """(there is no device here: a call that reached the library would raise RuntimeError)"""
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(TypeError, match="interp"):
        precon.multigrid(ll(6), (7,), galerkin=True, interp=bad)  # before the grid is looked at
    with pytest.raises(TypeError, match="interp"):
        device.DeviceMultigridInterp(fake_csr((6, 6)), (7,), interp=bad)


@pytest.mark.parametrize("bad", ["Operator", "dendy", "bilinear", ""])
def test_an_unknown_interp_is_a_value_error(bad):
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match="interp"):
        precon.multigrid(ll(6), (6,), galerkin=True, interp=bad)
    with pytest.raises(ValueError, match="interp"):
        device.DeviceMultigridInterp(fake_csr((6, 6)), (6,), interp=bad)


def test_operator_needs_galerkin_and_takes_no_line_and_no_single():
    from pysparse.precon import precon
    from pysparse_amd import device
    for kw in ({}, {"galerkin": False}):
        with pytest.raises(ValueError, match="galerkin=True"):
            precon.multigrid(ll(6), (6,), interp="operator", **kw)
    with pytest.raises(ValueError, match="galerkin=True"):
        device.DeviceMultigridInterp(fake_csr((6, 6)), (6,), galerkin=False)
    with pytest.raises(ValueError, match="not supported"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, line=0, interp="operator")
    with pytest.raises(ValueError, match="not supported"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, precision="single", interp="operator")
    with pytest.raises(ValueError, match="not supported"):
        precon.multigrid(ll(6), (2, 3), galerkin=True, precision="single", stencil="box", interp="operator")
    new = object.__new__
    with pytest.raises(ValueError, match="not supported"):
        device.DeviceMultigrid._create(new(device.DeviceMultigridInterp), fake_csr((6, 6)), (2, 3), 0.8, 2, True, 0, "axis", "operator")
    with pytest.raises(ValueError, match="not supported"):
        device.DeviceMultigrid._create(new(device.DeviceMultigrid32), fake_csr((6, 6)), (2, 3), 0.8, 2, True, None, "axis", "operator")


@pytest.mark.parametrize("good,kw", [("linear", {}), ("linear", {"galerkin": True}), ("operator", {"galerkin": True}),
                                     ("linear", {"galerkin": True, "precision": "single"}),
                                     ("operator", {"galerkin": True, "stencil": "box"})])
def test_valid_strings_pass_the_parser(good, kw):
    """what surfaces is the ValueError of the later checks, which do not mention the keyword"""
    from pysparse.precon import precon
    from pysparse_amd import device
    with pytest.raises(ValueError, match="grid") as e:
        precon.multigrid(ll(6), (7,), interp=good, **kw)
    assert "interp" not in str(e.value)
    with pytest.raises(ValueError, match="omega"):
        precon.multigrid(A=ll(6), grid=(6,), omega=2.0, steps=2, interp=good, **kw)
    if good == "operator":
        kw = {k: v for k, v in kw.items() if k != "precision"}
        with pytest.raises(ValueError, match="grid"):
            device.DeviceMultigridInterp(fake_csr((6, 6)), (7,), **kw)
        with pytest.raises(ValueError, match="steps"):
            device.DeviceMultigridInterp(fake_csr((6, 6)), (6,), 0.8, 0, **kw)


def test_device_multigrid_interp():
    from pysparse_amd import device
    assert issubclass(device.DeviceMultigridInterp, device.DeviceMultigrid)
    p = inspect.signature(device.DeviceMultigridInterp.__init__).parameters
    assert list(p)[1:] == ["A", "grid", "omega", "steps", "galerkin", "stencil", "interp"]
    assert p["galerkin"].default is True and p["stencil"].default == "axis" and p["interp"].default == "operator"
    # DeviceMultigrid's signature is untouched
    assert list(inspect.signature(device.DeviceMultigrid.__init__).parameters)[1:] == ["A", "grid", "omega", "steps", "galerkin"]
    assert device.PSP_MG_INTERP == 16
    assert device.PSP_MG_INTERP not in (device.PSP_MG_GALERKIN, device.PSP_MG_SINGLE, device.PSP_MG_BOX, 4)
    assert isinstance(device.DeviceMultigrid.interp, property) and device.DeviceMultigrid.interp.fset is None
    assert hasattr(device.DeviceMultigrid, "transfer_weights") and hasattr(device.DeviceMultigrid, "interp_fallbacks")


def test_the_drop_in_type_has_a_read_only_interp():
    from pysparse.precon import precon
    d = precon.MultigridType.__dict__["interp"]
    assert type(d).__name__ == "getset_descriptor" and "'linear' or 'operator'" in d.__doc__


NEW_SYMBOLS = ("psp_mg_interp", "psp_mg_interp_fallbacks", "psp_mg_transfer_weights")


def test_new_symbols_are_declared_and_exported():
    from pysparse_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pysparse_hip.h")) as f:
        header = f.read()
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in _capi.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name  # bound with a signature, not only exported
    assert "#define PSP_MG_INTERP 16u" in header
    assert "int psp_mg_interp(const psp_mg_t *K, int *operator_dependent);" in header
    assert "int psp_mg_interp_fallbacks(psp_mg_t *K, int level, long long *points);" in header
    assert "int psp_mg_transfer_weights(psp_mg_t *K, int level, int *nslots_inout, double *W_host);" in header


# ------------------------------------------------------------------------------------------------ oracle guards

def test_extended_precision_is_there():
    assert np.finfo(LD).eps < 1e-18


def test_block_kappa():
    k = block_kappa((13, 11), 3, 1e6, 0.4, 0)
    assert k.shape == (13, 11) and set(np.unique(k)) == {1.0, 1.0e6}
    assert np.array_equal(k, block_kappa((13, 11), 3, 1e6, 0.4, 0)) and not np.array_equal(k, block_kappa((13, 11), 3, 1e6, 0.4, 1))
    assert np.all(k[:3, :3] == k[0, 0]) and np.all(k[3:6, 9:11] == k[3, 9])
    A = interp_operator((11, 13), "b3_1e6")
    assert abs(A - A.T).max() == 0.0 and A.diagonal().min() > 0.0
    assert abs(interp_operator((5, 6), "const") - varying_operator((5, 6), "const")).max() == 0.0


@pytest.mark.parametrize("n", [7, 8, 64])
def test_constant_coefficients_in_one_dimension_give_half_and_one(n):
    O = interp_oracle_for((n,), "const")
    for g, W in zip(O.grids, O.W):
        i = np.arange(g[0])
        odd = i % 2 == 1
        assert np.array_equal(W[0, odd], np.ones(odd.sum())) and np.array_equal(W[1, odd], np.zeros(odd.sum()))
        assert np.array_equal(W[0, ~odd], np.where(i[~odd] >= 2, 0.5, 0.0))
        assert np.array_equal(W[1, ~odd], np.where(i[~odd] // 2 < g[0] // 2, 0.5, 0.0))
    L = linear_oracle_for((n,), "const")
    for P, Q in zip(O.P, L.P):
        assert abs(P - Q).max() == 0.0


@pytest.mark.parametrize("grid,s,want", [((9, 7), 0.0, 6), ((10, 9, 8), 0.3, 7)])
def test_constant_coefficients_converge_like_the_linear_cycle(grid, s, want):
    """the table's last row: 6 / 7 iterations with either interpolation, the counts this oracle gives"""
    A, b = interp_operator(grid, "const", s), rhs(grid, 3)
    it = pcg_margin(A, b, 1e-8, 100, interp_oracle_for(grid, "const", s).apply)[0]
    itl = pcg_margin(A, b, 1e-8, 100, linear_oracle_for(grid, "const", s).apply)[0]
    print("constant kappa %s: %d iterations with operator-dependent interpolation, %d with linear" % (grid, it, itl))
    assert (it, itl) == (want, want)


@pytest.mark.parametrize("grid,kind", [((13, 11), "b3_1e4"), ((9, 7, 6), "b3_1e4"), ((13, 11), "box_b3_1e4")])
def test_oracle_cycle_is_symmetric_positive_definite(grid, kind):
    """the dense cycle with 1e4 blocks is symmetric to 1e-13 and all its eigenvalues are > 0"""
    n = int(np.prod(grid))
    O = interp_oracle_for(grid, kind)
    for omega, steps in ((0.8, 2), (1.0, 1)):
        M = np.column_stack([O.apply(e, omega, steps) for e in np.eye(n)])
        assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max(), (grid, kind)
        assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0.0, (grid, kind)



@pytest.mark.parametrize("grid,kind", [((13, 11), "b3_1e6"), ((9, 7, 6), "b3_1e6"), ((40, 5), "b4_1e4"), ((13, 11), "box_b3_1e6")])
def test_the_two_legs_agree(grid, kind):
    O = interp_oracle_for(grid, kind)
    b = rhs(grid, 3)
    for omega, steps in ((0.8, 2), (1.0, 1)):
        z, zx = O.apply(b, omega, steps), O.apply_ext(b, omega, steps)
        assert zx.dtype == LD
        e64 = np.abs(z - zx).max() / np.abs(zx).max()
        print("%s %s omega %.1f steps %d: the float64 leg is %.1f eps from the longdouble one" % (grid, kind, omega, steps, e64 / EPS))
        assert e64 <= 1e-9, (grid, kind)


@pytest.mark.parametrize("grid,kind", [((33, 17), "b3_1e6"), ((9, 7, 6), "b2_1e4"), ((40, 5), "b4_1e4")])
def test_level_operators_keep_the_box_and_the_level_grids(grid, kind):
    O = interp_oracle_for(grid, kind)
    assert O.grids == level_grids(grid)
    for g, A in zip(O.grids, O.A):
        C = A.tocoo()
        k, j = C.row, C.col
        for m in g:
            assert np.abs(k % m - j % m).max() <= 1
            k, j = k // m, j // m
    for P in O.P:  # a weight per parent, no more than 2^nd parents
        assert np.diff(P.indptr).max() <= 2 ** len(grid)


def test_prolongation_rows_sum_to_one_away_from_the_boundary_without_shift():
    """with s = 0 and constant row sums 0 in the interior, interpolation reproduces constants there"""
    O = interp_oracle_for((13, 11), "b3_1e6")
    P, g = O.P[0], O.grids[0]
    i = np.arange(P.shape[0])
    inner = (i % g[0] > 0) & (i % g[0] < g[0] - 1) & (i // g[0] > 0) & (i // g[0] < g[1] - 1)
    assert np.abs(np.asarray(P.sum(axis=1)).ravel()[inner] - 1.0).max() <= 64 * EPS


def test_the_fallback_branch_is_exercised():
    """at least one operator of the GPU comparisons has points that take the linear weights"""
    hit = [(g, k, interp_oracle_for(g, k, s, sd).fallbacks) for g, k, s, sd in GPU_CASES if int(np.prod(g)) <= 70 * 45]
    print([h for h in hit if sum(h[2])])
    assert any(sum(h[2]) > 0 for h in hit)


@pytest.mark.parametrize("grid,kind,s,seed", GPU_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_decision_margin(grid, kind, s, seed):
    """a condition on the inputs: at every point of every level |T0| > 1e-9 sum |T[delta]|, or all T are 0 -- the device and
    the oracle cannot disagree on the branch by rounding; and the two legs of the oracle take the same branches"""
    O = interp_oracle_for(grid, kind, s, seed)
    print(grid, kind, "margins", O.margin, "fallbacks", O.fallbacks)
    assert min(O.margin) > 1e-9
    assert O.fallbacks == O.fallbacks_ext


@pytest.mark.parametrize("key", sorted(PCG_TABLE), ids=lambda v: "%s-%s" % (v[0], "x".join(map(str, v[1]))))
def test_the_table_is_what_the_oracle_gives(key):
    kind, grid = key
    seed, want, wantl, wantj = PCG_TABLE[key]
    ops = OP_SEED.get(key, 0)
    A, b = interp_operator(grid, kind, 0.0, ops), rhs(grid, seed)
    it, last, before = pcg_margin(A, b, 1e-8, 3000, interp_oracle_for(grid, kind, 0.0, ops).apply)
    itl = pcg_margin(A, b, 1e-8, 3000, linear_oracle_for(grid, kind, 0.0, ops).apply)[0]
    dinv = 1.0 / A.diagonal()
    itj = pcg_margin(A, b, 1e-8, 3000, lambda r: dinv * r)[0]
    print("%s %s seed %d: PCG with interp='operator' %d iterations (stopping residual %.3f tol||b||, the one before %.3f), "
          "linear %d, Jacobi %d" % (kind, grid, seed, it, last, before, itl, itj))
    assert (it, itl, itj) == (want, wantl, wantj)
    for r in (last, before):
        assert not 0.9 <= r <= 1.1, "a residual within 10 % of the threshold: choose another seed"


@pytest.mark.parametrize("key", sorted(PCG_TABLE), ids=lambda v: "%s-%s" % (v[0], "x".join(map(str, v[1]))))
def test_unstable_rows_are_unstable_in_the_oracle_itself(key):
    """a row is in UNSTABLE iff the oracle's own solve misses a true residual of 1e-8 ||b||, or takes another number of
    iterations with its cycle evaluated in np.longdouble (rows of at most 16384 points and 60 iterations) or with the dot
    products of the loop summed in another order (reversed, in np.longdouble, two seeded permutations)"""
    kind, grid = key
    seed, want = PCG_TABLE[key][:2]
    ops = OP_SEED.get(key, 0)
    A, b, O = interp_operator(grid, kind, 0.0, ops), rhs(grid, seed), interp_oracle_for(grid, kind, 0.0, ops)
    it, x = oracle_pcg(A, b, 1e-8, 3000, O.apply)
    true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    assert it == want
    runs = [(it, x)]
    if b.size <= 16384 and want <= 60:
        runs.append(oracle_pcg(A, b, 1e-8, 3000, lambda r: O.apply_ext(r).astype(np.float64)))
    for v in (1, 2, 3, 4):
        runs.append(oracle_pcg_variant(A, b, 1e-8, 3000, O.apply, v))
    counts = sorted({r[0] for r in runs})
    worst = max(np.linalg.norm(b - A @ r[1]) / np.linalg.norm(b) for r in runs)
    print("%s %s: %d iterations, true residual %.3e ||b||; over the variations counts %s, worst true residual %.3e"
          % (kind, grid, it, true, counts, worst))
    unstable = true > 1e-8 or len(counts) > 1
    assert unstable == (key in UNSTABLE)
    if key in UNSTABLE:
        lo, hi, recorded = UNSTABLE[key]
        assert (counts[0], counts[-1]) == (lo, hi)
        assert 0.9 * recorded <= worst <= recorded  # the recorded figure is the measured one, rounded up
