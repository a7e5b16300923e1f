"""GPU against the reference's iterates AT BASELINE.json's OWN SIZES (configs[1] 4096^2, configs[2] 512^3).

tests/test_gpu_fullsize.py checks the full-size runs through properties and cross-kernel comparisons; the golden-size
tests pin every kernel to the oracle bit for bit / to 1e-12.  This file closes the gap in between: the same k
iterations (tol = 0, so exactly k run) of Jacobi-PCG (pysparse/itsolvers/src/pcg.c:91-163) and Jacobi-MINRES
(minres.c:96-193) on the SAME system (b = A*ones, x0 = 0)

  * by the oracle (oracle/pysparse_oracle.c, one core, sequential sums),
  * by the reference's own compiled kernels when oracle/_ref was built (it travels to the GPU box): the standalone
    examples/poisson_test/pcg.c, and the module's pcg.c and minres.c (libref_krylov.so, refk_solve) -- round 5 added
    MINRES against its own reference kernel,
  * on the GPU through the host-pointer entry points the drop-in modules call,

and requires equal (info, iter) and relres / max-norm of x within

  * GPU vs oracle:              bench.parity_bound(n, k)              = 32 k sqrt(n) eps
  * GPU vs compiled reference:  bench.parity_bound(n, k, "reference") =  4 k sqrt(n) eps   (round 5; 3.1e-11 at C3 / k = 3)

(eps = 2^-52) -- the size-dependent form of north_star's 1e-12: implementations that differ only in the order of their
dot-product sums drift apart like k sqrt(n) eps.  The oracle's one-after-the-other sums are the outlier (4.9e-11 from the
compiled reference at 512^3 / k = 3), hence the wider bar against it; the GPU's tree sums and OpenBLAS's blocked sums
were measured 1.3e-13 apart there (BENCH_r04), so 4x keeps ~200x head-room while an error of 1e-10 in a fused update
fails.  The long leg drives the COMPILED pcg.c / minres.c through k = 20 iterations at 512^3 with row-parallel operator
callbacks (same bits per row; the kernels are the reference's code) so that drift, not just the first steps, is
compared.  The short comparisons ride in every `bench.py --full` run as `parity_check`."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _mem_available_gb():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable"):
            return int(line.split()[1]) / 1e6
    return 0.0


def _check(out, k, with_oracle, need_ref):
    import bench
    n = out["n"]
    bound, bound_ref = bench.parity_bound(n, k), bench.parity_bound(n, k, "reference")
    assert out["bound"] == bound and out["bound_vs_reference"] == bound_ref
    assert bound_ref == bound / 8
    for name in ("pcg", "minres"):
        r = out[name]
        # tol = 0: PCG runs out with iter = maxit + 1 (pcg.c:165), MINRES stops at it_max (minres.c:114)
        want = [-1, k + 1] if name == "pcg" else [-1, k]
        assert r["info_iter_gpu"] == want, (name, r)
        if with_oracle:
            assert r["info_iter_oracle"] == want, (name, r)
            assert r["relres_rel_diff"] <= bound and r["x_max_rel_diff"] <= bound, (name, r)
        if need_ref:
            v = r["vs_reference_module_kernel"]  # pcg.c / minres.c of the extension module, compiled unmodified
            assert v["kernel"].endswith(name + ".c") and v["info_iter_reference"] == want, (name, v)
            assert v["x_max_rel_diff"] <= bound_ref and v["relres_rel_diff"] <= bound_ref, (name, v)
            if with_oracle:
                assert v["oracle_vs_reference_x_max_rel_diff"] <= bound  # the CPU-vs-CPU floor lies inside the wide bar
    if need_ref and "vs_reference_pcg" in out["pcg"]:
        v = out["pcg"]["vs_reference_pcg"]  # the standalone program's pcg.c
        assert v["info_iter_reference"] == [-1, k + 1]
        assert v["x_max_rel_diff"] <= bound_ref and v["relres_rel_diff"] <= bound_ref, v
    assert out["ok"]


@pytest.fixture(scope="module")
def c3_host(oracle):
    """the 512^3 operator and right-hand side on the host, shared by the two C3 tests below (generating them twice was 18 s
    of the suite); None where the box has no room"""
    if _mem_available_gb() < 64:
        yield None
        return
    A = oracle.poisson_csr(512, 512, 512)
    b = np.empty(A.shape[0])
    A.matvec(np.ones(A.shape[0]), b)
    yield A, b
    del A, b


@pytest.mark.parametrize("grid,k", [((4096, 4096, 0), 10), ((512, 512, 512), 3)])
def test_gpu_iterates_against_oracle_and_reference_at_baseline_sizes(oracle, grid, k, c3_host):
    import bench
    from pysparse_amd import device as dev
    if grid[2] and c3_host is None:
        pytest.skip("512^3 on the host (14 GB of matrix + vectors) needs more memory than this box has free")
    A, b = c3_host if grid[2] else (None, None)
    out = bench.gpu_parity_case(dev, oracle, grid, k, A=A, b=b)
    assert out["n"] == grid[0] * grid[1] * max(grid[2], 1)
    assert bench.parity_bound(out["n"], k) < 5e-10 and bench.parity_bound(out["n"], k, "reference") < 4e-11
    need_ref = oracle.have_ref() and oracle.have_ref_krylov()
    if need_ref:
        assert "vs_reference_pcg" in out["pcg"]
    _check(out, k, True, need_ref)


def test_gpu_against_compiled_reference_20_iterations_at_512_cubed(oracle, c3_host):
    """drift, not just the first steps: k = 20 at C3 against the reference's own pcg.c and minres.c (no oracle leg: its
    sequential products would take minutes; the compiled kernels get the row-parallel callbacks)"""
    import bench
    from pysparse_amd import device as dev
    if not (oracle.have_ref() and oracle.have_ref_krylov()):
        pytest.skip("oracle/_ref was not built (needs /root/reference at build time)")
    if c3_host is None:
        pytest.skip("512^3 on the host + the reference kernels' 8 n work array need more memory than this box has free")
    k = 20
    threads = bench._usable_cores()
    out = bench.gpu_parity_case(dev, oracle, (512, 512, 512), k, A=c3_host[0], b=c3_host[1], with_oracle=False,
                                ref_threads=threads)
    assert bench.parity_bound(out["n"], k, "reference") < 2.1e-10
    _check(out, k, False, True)
    for name in ("pcg", "minres"):
        assert out[name]["vs_reference_module_kernel"]["callback_threads"] == threads
    print("C3 k=20 vs compiled reference:", {nm: (out[nm]["vs_reference_module_kernel"]["x_max_rel_diff"],
                                                   out[nm]["vs_reference_module_kernel"]["seconds"]) for nm in ("pcg", "minres")})


@pytest.mark.parametrize("grid,k", [((1024, 1024, 0), 200), ((40, 40, 300), 120)])
def test_single_kernel_range_against_oracle_and_reference(oracle, grid, k):
    """2^18 < n <= 2^20: the product path is ONE cooperative kernel per solve (psp_mid.hip; tests/test_gpu_mid.py pins it
    bit for bit to the launch-per-phase loops) -- here the same solves against the oracle and the reference's compiled
    pcg.c / minres.c, hundreds of iterations deep"""
    import ctypes as C

    import bench
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    s0, f0, s1, f1 = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
    lib().psp_debug_mid_count(C.byref(s0), C.byref(f0))
    out = bench.gpu_parity_case(dev, oracle, grid, k)
    lib().psp_debug_mid_count(C.byref(s1), C.byref(f1))
    assert s1.value - s0.value >= 2 and f1.value == f0.value  # PCG and MINRES both ran as single kernels
    assert (1 << 18) < out["n"] <= (1 << 20)
    _check(out, k, True, oracle.have_ref() and oracle.have_ref_krylov())


@pytest.mark.parametrize("grid,k", [((4096, 4096, 0), 10), ((96, 96, 96), 60)])
def test_sss_form_against_oracle_and_reference(oracle, grid, k):
    """the same comparison with the operator held as an sss_mat on the GPU (sss_spmv_w4; in the single-kernel range the
    offset table of its mirror): SURVEY 8a row B2 at configs[1]'s size, in the single-kernel range and on a 3-D grid"""
    import bench
    from pysparse_amd import device as dev
    out = bench.gpu_parity_case(dev, oracle, grid, k, form="sss")
    assert out["form"] == "sss" and out["n"] == grid[0] * grid[1] * max(grid[2], 1)
    _check(out, k, True, oracle.have_ref() and oracle.have_ref_krylov())


def test_brick_range_against_oracle_and_reference(oracle):
    """3-D grids of 1.5e5 .. 2^20 points: the product path is ONE cooperative kernel with the points dealt out in bricks
    (psp_mid.hip; its sums are ordered differently from every other loop's) -- 100 iterations against the oracle and the
    reference's compiled pcg.c / minres.c"""
    import ctypes as C

    import bench
    from pysparse_amd import device as dev
    from pysparse_amd._capi import lib
    s0, f0, s1, f1 = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_longlong()
    lib().psp_debug_brick_count(C.byref(s0), C.byref(f0))
    out = bench.gpu_parity_case(dev, oracle, (80, 80, 80), 100)
    lib().psp_debug_brick_count(C.byref(s1), C.byref(f1))
    assert s1.value - s0.value >= 2 and f1.value == f0.value  # PCG and MINRES both ran in bricks
    _check(out, 100, True, oracle.have_ref() and oracle.have_ref_krylov())
