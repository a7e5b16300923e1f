"""Every fused vector pass of psp_vec.hip on its own, through psp_debug_vec_pass, at every form its launch can take.

The cgs / bicgstab / qmrs / gmres / minres passes and the Jacobi kernels otherwise run only inside whole solves, on
vectors from the library's aligned pool, at sizes below 4 * 10^4 or at 2^20.  Here each one is launched alone and compared
with its NumPy statement (tests/vec_passes_ref.py, which tests/test_vec_passes_host.py ties to the oracle):

  * vectors bit for bit (the passes are element-wise and built without FMA contraction), inputs unchanged, the doubles
    around every vector untouched;
  * every reduction against the same sum in np.longdouble, within 64 eps sum|a_i b_i|: a term passes through at most
    2 + 6 + 3 + 8 + 13 additions (thread, wave, workgroup, group of 256, group sums) and one product rounding, 33 roundings,
    and 64 is the margin the multigrid tests use.  Worst observed |sum - exact| / bound over all passes and sizes on the
    MI355X: 0.014, in lanczos at n = 4097 (printed per pass with -s);
  * sizes 1, 2, 513 (one element into the second span of 512), 1000, 4097 and 2^21 + 514 (4098 partial sums: the first
    size at which finish_partials folds by groups); without a preconditioner, with the dinv array, with a constant dinv
    unhinted and hinted;
  * with all buffers 16-byte aligned, all 8 bytes off, and each operand 8 bytes off alone: psp_debug_vec_form must report
    the 16-byte form exactly when n is even and every operand the running form dereferences is aligned (the table of
    vec_passes_ref.py, written from the kernels), and all results are the same bits in every one of these runs;
  * scalars taken from a device state (registers chosen here, NaN by value) give the bits of the by-value run, and a
    state whose status is set leaves every vector alone;
  * daxpy's quick return for a zero coefficient where the other operand holds inf.

Out of scope: the looping grid beyond kMaxParts workgroups (n > 2^30) needs 8 GB per vector."""
import ctypes as C

import numpy as np
import pytest

import vec_passes_ref as R

pytestmark = pytest.mark.gpu

GUARD, PAD = 777.0, 2
EPS = float(np.finfo(np.float64).eps)
BIG = (1 << 21) + 514
SIZES = [1, 2, 513, 1000, 4097, BIG]
# neither 0 nor +-1
SCALARS = {"a": 0.37, "b": -1.3, "alpha": 0.37, "beta": -1.3, "omega": 0.61, "cc": 0.83, "eta": -0.29, "rho1inv": 1.7,
           "c1": 0.41, "c2": -0.77, "r1": 1.9, "r2": -0.53, "r3": 0.27, "c_eta": 0.45, "vdiv": 2.3, "np_prev": 300.0}
WORST = {}


def _capi():
    from pysparse_amd import _capi
    return _capi


_pool_cache = {}


def _pool(n):
    """eight seeded normal vectors of length n, the dinv array and the constant one (computed once per size, never
    written: every run copies out of them)"""
    if n not in _pool_cache:
        if n == BIG or len(_pool_cache) > 8:
            _pool_cache.clear()
        rng = np.random.default_rng(n)
        vs = [rng.standard_normal(n) for _ in range(8)]
        _pool_cache[n] = (vs, 1.0 / (4.0 + rng.random(n)), np.full(n, 1.0 / 6.0))
        for a in vs + list(_pool_cache[n][1:]):
            a.setflags(write=False)
    return _pool_cache[n]


def host_vectors(name, n):
    vs, _, _ = _pool(n)
    host = {v: vs[k] for k, v in enumerate(R.PASSES[name]["vecs"])}
    if name == "axpy_dot_chain":
        host["prev"] = np.random.default_rng(3).standard_normal(int(SCALARS["np_prev"]))
        host["h_out"] = np.array([GUARD])
    return host


def scalars(name):
    return [SCALARS[s] for s in R.PASSES[name]["scal"]]


def variants(name):
    """(label, flags, reference keywords, operands handed over as NULL)"""
    K = _capi()
    if name == "bicg_p":
        return [("later", 0, {"first": False}, ()), ("first", K.VEC_FIRST, {"first": True}, ())]
    if name == "minres_wx":
        return [("plain", 0, {"scaled": False}, ()), ("scaled", K.VEC_SCALED, {"scaled": True}, ())]
    if name == "axpy_dot":
        return [("z", 0, {}, ()), ("self", 0, {}, ("z",)), ("coef_dev", K.VEC_COEF_DEV, {}, ())]
    if name == "axpy_dot_chain":
        return [("z", 0, {}, ()), ("self", 0, {}, ("z",))]
    return [("", 0, {}, ())]


def effective(label, scal):
    """the scalars the reference takes: the coefficient form of axpy_dot uses minus the value it is handed"""
    return [-scal[0]] if label == "coef_dev" else scal


def forms(name):
    P = R.PASSES[name]
    if P["pre"]:
        return ["none", "array", "constant", "hinted"]
    return ["array"] if P["dinv"] == "always" else ["none"]


_arena, _arena_used = {}, {}


def _buffer(count):
    from pysparse_amd import device as dev
    k = _arena_used.get(count, 0)
    have = _arena.setdefault(count, [])
    if k == len(have):
        have.append(dev.DeviceBuffer(count))
        assert have[-1].ptr % 16 == 0
    _arena_used[count] = k + 1
    return have[k]


@pytest.fixture(autouse=True)
def _free_the_arena():
    yield
    for bufs in _arena.values():
        for b in bufs:
            b.free()
    _arena.clear()


class Run:
    pass


def run(name, n, host, scal, form="none", mis=(), flags=0, regs=(0, 0, 0), it=0, alias=None, want_rc=0):
    """one psp_debug_vec_pass.  host: {operand: array or None (NULL)}; form: none / array / constant / hinted; mis: the
    operands (R.KDINV: the preconditioner's array) that start 8 bytes off a 16-byte boundary; alias: {operand: operand
    whose buffer it shares}.  -> Run with .vec (every vector as it is afterwards), .sums, .V, .pre, .rc"""
    K = _capi()
    L = K.lib()
    P = R.PASSES[name]
    _arena_used.clear()
    alias = alias or {}
    bufs, ptrs = {}, []
    for v in P["vecs"]:
        a = host.get(v)
        if v in alias:
            ptrs.append(ptrs[P["vecs"].index(alias[v])])
            continue
        if a is None:
            ptrs.append(None)
            continue
        off = PAD + (1 if v in mis else 0)
        full = np.full(len(a) + 2 * PAD + 1, GUARD)
        full[off:off + len(a)] = a
        b = _buffer(len(full))
        b.upload(full)
        bufs[v] = (b, off, len(a))
        ptrs.append(b.ptr + 8 * off)
    dptr, dh = None, None
    if form != "none":
        _, darr, dconst = _pool(n)
        dh = darr if form == "array" else dconst
        off = PAD + (1 if R.KDINV in mis else 0)
        full = np.full(n + 2 * PAD + 1, GUARD)
        full[off:off + n] = dh
        b = _buffer(len(full))
        b.upload(full)
        bufs[R.KDINV] = (b, off, n)
        dptr = b.ptr + 8 * off
    sums = _buffer(4)
    sums.upload(np.full(4, np.nan))
    vec = (C.c_void_p * len(ptrs))(*ptrs)
    sc = (C.c_double * max(1, len(scal)))(*scal)
    if form == "hinted":
        K.check(L.psp_k_hint_constant(dptr, n))
    try:
        rc = L.psp_debug_vec_pass(K.VEC_PASSES.index(name), n, vec, len(ptrs), dptr, sc if scal else None, len(scal),
                                  flags, regs[0], regs[1], regs[2], it, sums.ptr)
    finally:
        if form == "hinted":
            K.check(L.psp_k_unhint(dptr))
    out = Run()
    out.rc = rc
    assert rc == want_rc, (name, n, form, mis, rc, L.psp_last_error())
    V, pre = C.c_int(-1), C.c_int(-1)
    K.check(L.psp_debug_vec_form(C.byref(V), C.byref(pre)))
    out.V, out.pre = V.value, pre.value
    out.vec = {}
    for v, (b, off, m) in bufs.items():
        full = b.download()
        assert (np.delete(full, slice(off, off + m)) == GUARD).all(), (name, v, "wrote outside its vector")
        out.vec[v] = full[off:off + m].copy()
    out.sums = sums.download()[:P["nsums"]].copy()
    out.dinv = dh
    return out


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_values(name, n, host, scal, got, kw):
    """vectors equal the reference (NaN where it has NaN), inputs unchanged, sums within the bound -> worst ratio"""
    kw = dict(kw)
    if name == "axpy_dot_chain":
        prev = host["prev"].astype(np.longdouble)
        h = got.vec["h_out"][0]
        assert abs(h - prev.sum()) <= 64 * EPS * np.abs(prev).sum(), (name, n, "h_out")
        kw["h"] = h
    with np.errstate(all="ignore"):
        want, pairs = R.FUNCS[name](host, scal, got.dinv, **kw)
    for v, a in host.items():
        if a is None or v == "h_out" or v not in got.vec:
            continue
        w = want.get(v, a)
        assert np.array_equal(got.vec[v], w, equal_nan=True), (name, n, v, "written" if v in want else "an input changed")
    assert len(pairs) == len(got.sums)
    worst = 0.0
    for j, (a, b) in enumerate(pairs):
        prod = a.astype(np.longdouble) * b.astype(np.longdouble)
        exact, bound = prod.sum(), 64 * EPS * np.abs(prod).sum()
        err = abs(np.longdouble(got.sums[j]) - exact)
        assert err <= bound, (name, n, "sum %d" % j, float(got.sums[j]), float(exact), float(err), float(bound))
        if bound > 0:
            worst = max(worst, float(err / bound))
    return worst


def operands(name, host, form):
    """what can be moved 8 bytes on its own in this run"""
    ops = [v for v in R.PASSES[name]["vecs"] if host.get(v) is not None]
    return ops + ([R.KDINV] if form != "none" else [])


def expected_form(name, n, mis, form):
    P = R.PASSES[name]
    pre = {"none": 0, "array": 1, "constant": 1, "hinted": 2}[form] if P["pre"] else 0
    return (2 if R.takes_v2(name, n, mis, "constant" if form == "hinted" else "array" if form == "constant" else form)
            else 1), pre


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(R.PASSES))
def test_values(name, n):
    """(a): every vector and reduction against the reference, aligned and with every buffer 8 bytes off"""
    worst = 0.0
    for form in forms(name):
        if n == BIG and form in ("constant", "hinted"):
            continue
        for label, flags, kw, nulls in variants(name):
            host = host_vectors(name, n)
            for z in nulls:
                host[z] = None
            scal = scalars(name)
            for mis in ((), tuple(operands(name, host, form))):
                got = run(name, n, host, scal, form, mis, flags)
                assert (got.V, got.pre) == expected_form(name, n, mis, form), (name, n, form, label, mis)
                worst = max(worst, check_values(name, n, host, effective(label, scal), got, kw))
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print("vec pass %-16s n = %-8d worst |sum - exact| / bound = %.4f (all sizes so far: %.4f, all passes: %.4f)"
          % (name, n, worst, WORST[name], max(WORST.values())))


@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("name", list(R.PASSES))
def test_alignment_and_the_form_that_ran(name, n):
    """(b): aligned, all off, each operand off alone -- the form psp_debug_vec_form reports is the table's, and every
    result has the same bits in all of these runs and between the hinted and the unhinted constant"""
    for label, flags, kw, nulls in variants(name):
        host = host_vectors(name, n)
        for z in nulls:
            host[z] = None
        scal = scalars(name)
        first_of = {}
        for form in forms(name):
            ops = operands(name, host, form)
            seen = set()
            for mis in [(), tuple(ops)] + [(o,) for o in ops]:
                got = run(name, n, host, scal, form, mis, flags)
                want = expected_form(name, n, mis, form)
                assert (got.V, got.pre) == want, (name, n, form, label, mis, (got.V, got.pre), want)
                seen.add(got.V)
                key = "constant" if form == "hinted" else form
                if key not in first_of:
                    first_of[key] = got
                    check_values(name, n, host, effective(label, scal), got, kw)
                ref = first_of[key]
                for v in ref.vec:
                    assert same(got.vec[v], ref.vec[v]), (name, n, form, label, mis, v)
                assert same(got.sums, ref.sums), (name, n, form, label, mis, got.sums, ref.sums)
            assert seen == ({1, 2} if n % 2 == 0 else {1})


KRY = [name for name, P in R.PASSES.items() if P["kry"]]


@pytest.mark.parametrize("name", KRY)
def test_scalars_from_a_device_state(name):
    """(c): registers chosen here, NaN by value -> the bits of the by-value run; status set -> nothing changes"""
    K = _capi()
    assert len(KRY) == 9
    regs = (5, 29, 17)
    for n in (1000, 4097):
        host = host_vectors(name, n)
        scal = scalars(name)
        for form in ("none", "array") if R.PASSES[name]["pre"] else ("none",):
            cases = [(0, 7, 0)]
            if name == "bicg_p":  # `first` comes from iter == 1, whatever the flag says: (by-value flags, iter, DEVSCAL flags)
                cases = [(K.VEC_FIRST, 1, 0), (0, 2, K.VEC_FIRST)]
            for byval_flags, it, dev_flags in cases:
                ref = run(name, n, host, scal, form, (), byval_flags)
                got = run(name, n, host, scal, form, (), K.VEC_DEVSCAL | dev_flags, regs, it)
                assert (got.V, got.pre) == (ref.V, ref.pre)
                for v in ref.vec:
                    assert same(got.vec[v], ref.vec[v]), (name, n, form, it, v)
                assert same(got.sums, ref.sums), (name, n, form, it)
                off = run(name, n, host, scal, form, (), K.VEC_DEVSCAL | K.VEC_STATUS_SET | dev_flags, regs, it)
                for v, a in host.items():
                    assert same(off.vec[v], a), (name, n, form, v, "changed although the loop has ended")


def _with(a, idx, val):
    a = a.copy()
    a[idx] = val
    return a


@pytest.mark.parametrize("n", [1000, 4097])
def test_quick_returns(n):
    """(d): a zero coefficient leaves what netlib's daxpy leaves untouched, even against inf (0 * inf would be NaN) and for
    a -0.0 that an executed y + 0 * x would turn into +0.0; the sums are those of the untouched vector"""
    K = _capi()
    spots = [0, 1, n // 2, n - 1]

    def check(name, host, scal, flags=0, kw=None):
        for form in ("none", "array") if R.PASSES[name]["pre"] else ("none",):
            got = run(name, n, host, scal, form, (), flags)
            check_values(name, n, host, effective("coef_dev" if flags & K.VEC_COEF_DEV else "", scal), got, kw or {})
            yield got

    h = host_vectors("cgs_q", n)
    h["v"], h["x"] = _with(h["v"], spots, np.inf), _with(h["x"], spots, -0.0)
    for got in check("cgs_q", h, [0.0]):
        assert same(got.vec["x"], h["x"]) and same(got.vec["q"], h["u"])
    h = host_vectors("cgs_r", n)
    h["t"], h["r"] = _with(h["t"], spots, -np.inf), _with(h["r"], spots, -0.0)
    for got in check("cgs_r", h, [0.0]):
        assert same(got.vec["r"], h["r"]) and np.isfinite(got.sums).all()
    h = host_vectors("cgs_p", n)
    h["q"], h["p"] = _with(h["q"], spots, np.inf), _with(h["p"], spots, -np.inf)
    for got in check("cgs_p", h, [0.0]):
        assert same(got.vec["u"], h["r"]) and same(got.vec["p"], h["r"])
    for flags in (0, K.VEC_COEF_DEV):
        for self_form in (False, True):
            h = host_vectors("axpy_dot", n)
            h["x"], h["y"] = _with(h["x"], spots, np.inf), _with(h["y"], spots, -0.0)
            if self_form:
                h["z"] = None
            for got in check("axpy_dot", h, [0.0], flags):
                assert same(got.vec["y"], h["y"]) and np.isfinite(got.sums).all()
    h = host_vectors("axpy_dot_chain", n)
    h["x"], h["y"], h["prev"] = _with(h["x"], spots, np.inf), _with(h["y"], spots, -0.0), np.zeros(300)
    for got in check("axpy_dot_chain", h, [300.0]):
        assert got.vec["h_out"][0] == 0.0 and same(got.vec["y"], h["y"]) and np.isfinite(got.sums).all()


@pytest.mark.parametrize("n", [1000, 4097])
def test_lin2_in_place(n):
    """(e): z may be x or y"""
    host = host_vectors("lin2", n)
    a, b = scalars("lin2")
    want = a * host["x"] + b * host["y"]
    for target, other in (("x", "y"), ("y", "x")):
        got = run("lin2", n, dict(host, z=None), [a, b], alias={"z": target})
        assert np.array_equal(got.vec[target], want) and same(got.vec[other], host[other])


@pytest.mark.parametrize("n", [1000, 4097])
def test_dinv_on_a_singular_diagonal(n):
    """(e): dinv = omega / diag, infinities included; the count is that of the entries with 1 + d == 1"""
    host = host_vectors("dinv", n)
    d = host["diag"].copy()
    special = [0.0, -0.0, 1e-17, 5e-324, -1e-17, 3.0]
    d[:len(special)] = special
    d[n - 1] = 0.0
    host["diag"] = d
    omega = 0.37
    for mis in ((), ("diag", "dinv")):
        got = run("dinv", n, host, [omega], mis=mis)
        with np.errstate(all="ignore"):
            want = omega / d
        assert np.array_equal(got.vec["dinv"], want) and same(got.vec["diag"], d)
        assert want[0] == np.inf and want[1] == -np.inf and want[3] == np.inf
        assert got.sums[0] == float((1.0 + d == 1.0).sum()) == 6.0


@pytest.mark.parametrize("n", [1000, 4097])
def test_jacobi_sweep(n):
    """(e): preconmodule.c:50-51, y = (x - y) dinv + temp"""
    host = host_vectors("jacobi_sweep", n)
    got = run("jacobi_sweep", n, host, [], "array")
    assert np.array_equal(got.vec["y"], (host["x"] - host["y"]) * got.dinv + host["temp"])
    assert same(got.vec["x"], host["x"]) and same(got.vec["temp"], host["temp"]) and same(got.vec[R.KDINV], got.dinv)


@pytest.mark.parametrize("np_prev", [1, 255, 256, 257, 4096])
def test_chain_adds_the_partial_sums_as_the_finishing_kernel_does(np_prev):
    """(e): the chain step adds the partial sums the step before left, inside every workgroup: h_out has the bits
    finish_partials gives for the same partial sums (psp_k_dot on the same data: the same products in the same order)"""
    K = _capi()
    L = K.lib()
    m = 512 * np_prev
    big = host_vectors("axpy_dot", m)
    # the finished sum of y . z
    dot = run("qmrs_v", 1, {"t": np.ones(1), "v1": np.ones(1)}, [0.5])  # (any reducing pass: leaves ONE partial sum)
    by, bz, out = _buffer(m + 1), _buffer(m + 2), _buffer(4)
    by.upload(np.append(big["y"], GUARD))
    bz.upload(np.append(big["z"], [GUARD, GUARD]))
    K.check(L.psp_k_dot(m, by.ptr, bz.ptr, out.ptr))
    h_want = out.download()[0]
    # a stale count is refused: the last reducing pass left one partial sum, not np_prev
    small = host_vectors("axpy_dot_chain", 1000)
    small["prev"] = None
    if np_prev != 1:
        run("axpy_dot_chain", 1000, small, [float(np_prev)], flags=K.VEC_PREV_WS, want_rc=-1)
    # axpy_dot with a zero coefficient leaves y alone and y . z in np_prev partial sums
    step = run("axpy_dot", m, big, [0.0])
    assert same(step.vec["y"], big["y"]) and step.sums[0] == h_want
    got = run("axpy_dot_chain", 1000, small, [float(np_prev)], flags=K.VEC_PREV_WS)
    assert got.vec["h_out"][0] == h_want
    check_values("axpy_dot_chain", 1000, dict(small, prev=np.array([h_want])), [1.0], got, {})


def test_chain_refuses_counts_it_cannot_add():
    """(e): np_prev = 0 and 4097 are PSP_EINVAL and nothing is launched"""
    K = _capi()
    host = host_vectors("axpy_dot_chain", 1000)
    host["prev"] = np.zeros(4100)
    for bad in (0.0, 4097.0, 2.5, -1.0, float("nan")):
        got = run("axpy_dot_chain", 1000, host, [bad], want_rc=-1)
        for v, a in host.items():
            assert same(got.vec[v], a)
    # from the workspace: 4097 partial sums of a preceding pass are one too many
    m = 512 * 4097
    big = host_vectors("axpy_dot", m)
    step = run("axpy_dot", m, big, [0.0])
    assert np.isfinite(step.sums[0])
    host["prev"] = None
    got = run("axpy_dot_chain", 1000, host, [4097.0], flags=K.VEC_PREV_WS, want_rc=-1)
    assert same(got.vec["y"], host["y"]) and got.vec["h_out"][0] == GUARD


def test_argument_refusals():
    """(e): a wrong call ends as PSP_EINVAL before anything is launched"""
    K = _capi()
    L = K.lib()
    n = 1000
    one = _buffer(8)
    sc = (C.c_double * 5)(0.5, 0.5, 0.5, 0.5, 0.5)
    vec = (C.c_void_p * 8)(*[one.ptr] * 8)
    call = L.psp_debug_vec_pass
    assert call(-1, 4, vec, 3, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1
    assert call(len(K.VEC_PASSES), 4, vec, 3, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1
    assert b"unknown pass" in L.psp_last_error()
    lin2 = K.VEC_PASSES.index("lin2")
    assert call(lin2, 4, vec, 2, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1      # nvec
    assert call(lin2, 4, vec, 3, None, sc, 1, 0, 0, 0, 0, 0, one.ptr) == -1      # nscal
    assert call(lin2, 0, vec, 3, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1      # n
    assert call(lin2, -5, vec, 3, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1
    assert call(lin2, 4, None, 3, None, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1     # no vector list
    assert call(lin2, 4, vec, 3, None, None, 2, 0, 0, 0, 0, 0, one.ptr) == -1    # no scalars
    assert call(lin2, 4, vec, 3, one.ptr, sc, 2, 0, 0, 0, 0, 0, one.ptr) == -1   # takes no dinv
    for flag in (K.VEC_FIRST, K.VEC_SCALED, K.VEC_DEVSCAL, K.VEC_STATUS_SET, K.VEC_COEF_DEV, K.VEC_PREV_WS, 64):
        assert call(lin2, 4, vec, 3, None, sc, 2, flag, 0, 1, 2, 0, one.ptr) == -1
    assert call(lin2, 4, vec, 3, None, sc, 2, 0, 0, 0, 0, 0, None) == 0           # reduces nothing: sums_dev ignored
    cgs_r = K.VEC_PASSES.index("cgs_r")
    assert call(cgs_r, 4, vec, 3, None, sc, 1, 0, 0, 0, 0, 0, None) == -1         # reduces: needs sums_dev
    assert call(cgs_r, 4, vec, 3, None, sc, 1, K.VEC_STATUS_SET, 0, 0, 0, 0, one.ptr) == -1
    assert call(cgs_r, 4, vec, 3, None, sc, 1, K.VEC_DEVSCAL, 32, 0, 0, 0, one.ptr) == -1
    assert call(cgs_r, 4, vec, 3, None, sc, 1, K.VEC_DEVSCAL, -1, 0, 0, 0, one.ptr) == -1
    dx = K.VEC_PASSES.index("qmrs_dx")
    assert call(dx, 4, vec, 5, None, sc, 3, K.VEC_DEVSCAL, 3, 4, 3, 0, one.ptr) == -1   # a register named twice
    assert call(K.VEC_PASSES.index("jacobi_sweep"), 4, vec, 3, None, None, 0, 0, 0, 0, 0, 0, None) == -1  # needs dinv
    # a NULL vector: refused where the selected form dereferences it, accepted where it does not
    for name, P in R.PASSES.items():
        host = host_vectors(name, n)
        form = "array" if P["dinv"] == "always" else "none"
        for v in P["vecs"]:
            free = v in P["with_pre"] or (v == "z" and name.startswith("axpy_dot"))
            got = run(name, n, dict(host, **{v: None}), scalars(name), form, want_rc=0 if free else -1)
            if not free:
                for u, a in host.items():
                    if u != v:
                        assert same(got.vec[u], a), (name, v, u)
        for v in P["with_pre"]:
            run(name, n, dict(host, **{v: None}), scalars(name), "array", want_rc=-1)
    V, pre = C.c_int(), C.c_int()
    assert L.psp_debug_vec_form(None, C.byref(pre)) == -1 and L.psp_debug_vec_form(C.byref(V), None) == -1
