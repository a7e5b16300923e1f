/*
 * pysparse_hip.h -- C ABI of libpysparse_hip.so, the MI355X (gfx950) implementation of
 * PySparse's SpMV + Krylov hot path.
 *
 * Plain C: ints, doubles, raw pointers and opaque handles only -- no Python, NumPy or
 * torch types cross this boundary.  The CPython extension modules in pysparse_amd/
 * (spmatrix, krylov, precon), bench.py and the GPU tests all go through these entry
 * points.  Citations are file:line under the reference tree (PythonOptimizers/pysparse).
 *
 * Conventions
 *   - every function returns PSP_OK (0) or a negative PSP_E* status; psp_last_error()
 *     returns the message of the calling thread's last failure.  Nothing throws.
 *   - "host" pointers are ordinary process memory, borrowed for the call;
 *     "dev" pointers are HIP device memory on the library's current device.
 *   - handles own their device memory; destroy releases it.
 *   - all work is enqueued on ONE stream (psp_set_stream; default = the null stream);
 *     host-pointer entry points synchronise before returning, *_dev entry points that
 *     return no scalar do not.
 *   - handles are not thread-safe; there is NO CPU fallback: without a usable GPU every
 *     compute entry point fails with PSP_ENODEV.
 *   - indices are 32-bit (the reference's C int: csr_mat.h:6-13), values are double.
 */
#ifndef PYSPARSE_HIP_H
#define PYSPARSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSP_OK 0
#define PSP_EINVAL (-1)   /* bad argument (shape, NULL, range)                     */
#define PSP_ENODEV (-2)   /* no HIP device / runtime error                         */
#define PSP_ENOMEM (-3)   /* device or host allocation failed                      */
#define PSP_ESINGULAR (-4) /* jacobi: diagonal element close to zero               */
#define PSP_ECALLBACK (-5) /* a host operator callback reported failure            */

/* solver info codes: pysparse/itsolvers/src/itsolversmodule.c:625-646 */
#define PSP_INFO_CONVERGED 0
#define PSP_INFO_MAXIT (-1)
#define PSP_INFO_ILLCOND_PRECON (-2)
#define PSP_INFO_NOT_SPD_PRECON (-3)
#define PSP_INFO_STAGNATION (-5)
#define PSP_INFO_BREAKDOWN (-6)

typedef struct psp_csr psp_csr_t;       /* device mirror of CSRMatObject, csr_mat.h:6-13     */
typedef struct psp_sss psp_sss_t;       /* device mirror of SSSMatObject, sss_mat.h:6-14     */
typedef struct psp_jacobi psp_jacobi_t; /* device mirror of JacobiObject, preconmodule.c:11-19 */
typedef struct psp_mg psp_mg_t;         /* precon.multigrid: matrix-free V-cycle; no reference analogue */
typedef struct psp_ssor psp_ssor_t;     /* device mirror of SSORObject, preconmodule.c:21-31   */
typedef struct psp_op psp_op_t;         /* "anything with shape + matvec / precon":
                                           the operator protocol of spmatrixmodule.c:169-248 */

/* ------------------------------------------------------------------ runtime */

const char *psp_last_error(void);
const char *psp_version(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int psp_device_count(void);
/* Threading: device, stream, reduction workspace and host staging belong to the CALLING THREAD.  The first thread
 * that uses the library enqueues on the null stream (or on what it hands psp_set_stream); every other thread gets a
 * non-blocking stream of its own on first use, so two threads with two handles overlap on the GPU.  A handle may be
 * shared between threads: every entry point locks the handles it is given (operator, preconditioner and the matrix
 * behind it), so calls on the SAME handle take turns.  (The reference holds the GIL across its whole solve.) */
/* select the device the calling thread's later calls use (hipSetDevice); threads that first call the library later
 * start on the device selected last */
int psp_set_device(int device);
/* which context the calling thread has: its slot (0 = the first thread), its device and the stream it enqueues on */
int psp_thread_info(int *thread_slot, int *device, void **hip_stream);
/* test hook of the locking discipline (tests/test_threading_cpu.py): takes the locks of the two handles exactly as an
 * entry point that is handed them does (address order, recursive), holds them for `milliseconds`, releases them */
int psp_debug_hold_handles(const void *h1, const void *h2, int milliseconds);
/* test hooks of the multi-stream ordering (tests/test_gpu_shake.py; only in a process started with PSP_TUNING=1, else
 * PSP_EINVAL).  psp_debug_shake arms delay injection: at every cut point of the multi-device driver whose bit is set in
 * point_mask (psp_internal.h ShakePoint), for every rank whose bit is set in rank_mask, a one-wave spin kernel of
 * min_us..max_us microseconds (pseudo-random from `seed`; a fixed delay when min_us == max_us) is enqueued on the stream
 * that cut point names, so that stream's later work moves against every other stream.  revert_mask takes a known fix
 * out again (bit 0: the copy stream's wait for the receiver's own stream, round 4) -- the test that the facility
 * finds what it is there to find.  seed < 0 disarms.  psp_debug_shake_count: spin kernels injected since it was armed.
 * psp_debug_spin: one spin kernel on the calling thread's stream (the torch driver's cut points, distributed.py). */
/* how many solves the single-kernel loop for mid-size offset-structured systems (psp_mid.hip) has run in this process,
 * and how many times it handed a solve back to the launch-per-phase loops (tests) */
int psp_debug_mid_count(long long *solves, long long *fallbacks);
/* the same counters for the brick form of those loops (7-offset operators of 3-D grids; psp_mid.hip) */
int psp_debug_brick_count(long long *solves, long long *fallbacks);
/* the device memory the handles of this process own through their array type (psp_internal.h DevArray: precon.ssor and
 * precon.multigrid handles with their set-up temporaries, the staging of csr_mat's host-pointer diagonal and transposed
 * product): bytes held now, and allocations made so far.  A handle that is closed gives back what it took, whether or not
 * psp_trim is called; the solvers' vector pool, the placement draws and the per-thread workspaces are not counted */
int psp_debug_device_bytes(long long *live_bytes, long long *allocations);
int psp_debug_shake(long long seed, int min_us, int max_us, unsigned point_mask, unsigned rank_mask, int revert_mask);
int psp_debug_shake_count(long long *injected);
int psp_debug_spin(int microseconds);
/* *can_access = 1 when `device` can read / write `peer`'s memory directly (xGMI or PCIe peer path; what the
 * halo copies of a multi-device matrix need), 1 for device == peer.  Creates no context: bench.py's pre-flight
 * matrix of an N-GPU run */
int psp_peer_access(int device, int peer, int *can_access);
/* Placement of library-owned vectors (round 5; pysparse_amd/csrc/psp_place.hip).  What a
 * bandwidth-bound product takes depends on which pages of HBM its vector operands occupy (two levels ~8 % apart at
 * 512^3); for the vectors the LIBRARY allocates -- the solvers' work vectors (the reference's solvers own their work
 * array too: pysparse/itsolvers/src/itsolversmodule.c:32-118) and the staging pair of the host-pointer products -- it
 * can draw a few candidates once per (device, length), time the handle's own product on each and keep the best.  Results
 * do not change by a bit.  psp_set_placement(1) turns the draws on; the default is OFF: measured over 11 processes the
 * product on a drawn pair is 0 ... 4.6 % faster (mean 1.8 %), Jacobi-PCG +0.5 ... +1.7 %, for 60-80 ms per draw
 * (profiles/r5_placement_ab_*.jsonl).  psp_placement_info: draws made so far and the milliseconds they took.  psp_place_operands hands the same service to a caller that owns its vectors:
 * *y_dev / *x_dev receive zeroed device vectors (nrows / ncols doubles, release with psp_free) chosen for the output /
 * input role of y = A x; report6 (may be NULL): candidates drawn (0: plain allocations -- vectors under 64 MiB, or memory
 * short), best and worst output-role ms, best and worst input-role ms, ms the draw took. */
int psp_set_placement(int on);
int psp_placement_info(int *enabled, long long *draws, double *draw_ms_total);
int psp_place_operands(const psp_csr_t *A, double **y_dev, double **x_dev, double *report6);
/* the calling thread enqueues on an externally owned hipStream_t (e.g. torch's current stream); NULL = null stream */
int psp_set_stream(void *hip_stream);
int psp_synchronize(void);
/* name, CU count and HBM bytes of the current device */
int psp_device_info(char *name, int name_len, int *compute_units, int64_t *hbm_bytes);
/* free / total device memory right now (leak checks; psp_trim() first to drop the solver scratch pool) */
int psp_mem_info(int64_t *free_bytes, int64_t *total_bytes);

/* device memory + timing hooks used by bench.py and the tests */
int psp_malloc(void **dev, size_t bytes);
int psp_free(void *dev);
int psp_memcpy_h2d(void *dev, const void *host, size_t bytes);
int psp_memcpy_d2h(void *host, const void *dev, size_t bytes);
int psp_memset(void *dev, int byte, size_t bytes);
/* release the cached solver work vectors (the library keeps the last few GB-sized scratch
 * vectors between solves because hipMalloc/hipFree of them costs milliseconds) */
int psp_trim(void);
int psp_event_create(void **event);
int psp_event_destroy(void *event);
int psp_event_record(void *event);                       /* on the library stream */
int psp_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
/* measurement hook ("timing hooks (hipEvent ms, bytes moved)"): what this GPU's memory
 * system gives a plain streaming kernel of a given shape right now, in THIS process -- `reads` (0..8) read
 * streams and `writes` (0..1) write streams of bytes_per_stream bytes each (a multiple of 4096), one 16-byte
 * element per thread and stream, one workgroup per 4 KiB span, `reps` timed launches after two untimed ones.
 * reads = 7, writes = 1 is the access shape of csr_spmv_w4 on the 7-point operator without its x re-reads:
 * bench.py prints it beside the SpMV as the ceiling of that shape.  The buffers are the call's own. */
int psp_stream_probe(int reads, int writes, size_t bytes_per_stream, int reps, float *avg_ms, float *min_ms);
/* Which loop the calling thread's LAST psp_pcg / psp_minres ran (the reference has one loop each: pcg.c:91-163,
 * minres.c:96-193; here the size and the operator pick one of several with the same semantics), so that a caller -- bench.py
 * -- derives its byte model from what ran instead of mirroring the selection rules.  name: "pcg_lazy_pf" (p and x updates
 * folded into the product: 4 launches), "pcg_lazy" (5), "pcg_eager" (6), "pcg_mid" / "pcg_brick" / "pcg_coop" (the whole
 * loop in one cooperative kernel), "pcg_host_scalars" (generic operands, Python callbacks), "minres_async", "minres_mid",
 * "minres_brick", "minres_coop", "minres_host_scalars", "pcg_multi" / "minres_multi" (device list); "" before the first
 * solve.  info[4] = {launches per iteration, vector bytes per row and iteration beside the product (0 inside the
 * single-kernel loops, -1 where not modelled), 1 when the Jacobi diagonal is streamed (not a constant), single-kernel
 * loops refused or abandoned after launch in this process so far (each fell back to the launch-per-phase loop)}. */
int psp_last_solve_info(char *name, int name_cap, int *info);
/* on = 0: psp_pcg / psp_minres never take the single-kernel loops (psp_mid.hip, psp_coop.hip) in this process.  Why one
 * would: the brick and small-system loops add their dot products in an order of their own that depends on the device's CU
 * count, so their iterates agree with the launch-per-phase loops' to rounding only, and a refused cooperative launch
 * (a shared GPU) falls back to those loops' bits -- with 0 every solve has the launch-per-phase bits on every device.
 * Default 1. */
int psp_set_single_kernel_loops(int on);
/* hash of the sources this binary was built from (__graft_entry__.source_hash(); "unstamped" for a hand build):
 * tests compare it with the hash of the sources on disk, so a stale prebuilt library cannot pass for a fresh one */
const char *psp_build_id(void);

/* ------------------------------------------------------------------ csr_mat */

/* replaces newCSRMatObject + the fill loop of LLMat_to_csr
 * (pysparse/sparse/src/csr_mat.c:259-296, ll_mat.c:1577-1648): uploads a host CSR
 * triple.  ind has nrows+1 entries, ind[0] == 0, ind[nrows] == nnz. */
int psp_csr_create(int nrows, int ncols, int nnz, const int *ind_host, const int *col_host,
                   const double *val_host, psp_csr_t **out);
/* scalable constructor: 5-/7-point Poisson operator generated ON the
 * device in the ordering of pysparse/tools/poisson.py:22-37, k = i + nx*j (+ nx*ny*l),
 * diag 4 (nz == 0, 2-D) or 6 (3-D), off-diagonals -1, columns ascending.
 * The slab form keeps only global rows [row_lo, row_hi) and shifts column indices by
 * -col_shift (row-range partition for multi-GPU; ncols_local = width of the local
 * extended x vector).  psp_csr_poisson == slab over all rows with shift 0. */
int psp_csr_poisson(int nx, int ny, int nz, psp_csr_t **out);
int psp_csr_poisson_slab(int nx, int ny, int nz, int64_t row_lo, int64_t row_hi, int64_t col_shift,
                         int ncols_local, psp_csr_t **out);
/* The same operator for grids whose nonzero count exceeds 32 bits (1024^3 on ONE GPU: 7.5e9
 * entries, the strong-scaling baseline of BASELINE.json configs[3]): generated directly in the
 * index-free offset-major layout of csr_spmv_w4, ~62 GB at 1024^3.  Supports
 * matvec, jacobi, the solvers and kernel_info; there are no CSR arrays to download or transpose.
 * psp_csr_shape reports nnz = -1 when it does not fit an int: use psp_csr_nnz64. */
int psp_csr_poisson_big(int nx, int ny, int nz, psp_csr_t **out);
/* Row slab [row_lo, row_hi) of the same index-free operator, columns shifted by -col_shift into a
 * local extended vector of ncols_local entries (same meaning as psp_csr_poisson_slab): the
 * strong-scaling legs of configs[3] at 2 and 4 GPUs hold 2^29 / 2^28 rows = 3.8e9 / 1.9e9 nonzeros
 * per rank, beyond 32-bit CSR offsets.  psp_csr_poisson_big == slab over all rows with shift 0. */
int psp_csr_poisson_big_slab(int nx, int ny, int nz, int64_t row_lo, int64_t row_hi, int64_t col_shift,
                             int ncols_local, psp_csr_t **out);
int64_t psp_csr_nnz64(const psp_csr_t *A);
/* Multi-GPU variants taking a device list (reference loops pcg.c:91-163,
 * minres.c:96-193, csr_mat.c:49-54): the rows of the operator -- and the matching slices of every solver
 * vector -- live as contiguous row blocks on devices[0..ndev), one rank per entry, ONE process (one host
 * thread enqueues for all ranks; a device may be listed more than once: ranks sharing a GPU).  The result is
 * an ordinary psp_csr_t: psp_csr_matvec(_stride), psp_csr_diagonal, psp_csr_shape, psp_csr_kernel_info,
 * psp_op_from_csr, psp_jacobi_create_csr (steps = 1), psp_pcg and psp_minres accept it -- K = NULL or the
 * jacobi of the same matrix -- and every other entry point answers PSP_EINVAL.  Ghost entries travel by peer
 * copies on a second stream per rank, overlapped with the rows that need none; the two packed reductions of
 * an iteration go through RCCL (ncclAllReduce in stream order; librccl is loaded on first use) when every
 * rank has its own device, else through a fixed-order fold kernel over peer pointers.
 *   poisson: z-slabs (y-slabs in 2-D) of whole grid planes, index-free slab operators (psp_csr_poisson_big_slab)
 *   create : any square CSR matrix from host arrays, n / ndev rows per rank, ghost lists found here */
int psp_csr_poisson_multi(int nx, int ny, int nz, const int *devices, int ndev, psp_csr_t **out);
int psp_csr_create_multi(int nrows, int ncols, int nnz, const int *ind_host, const int *col_host,
                         const double *val_host, const int *devices, int ndev, psp_csr_t **out);
/* ranks / distinct devices behind a handle (0 / 0 for a single-device matrix); uses_rccl: the reductions go
 * through RCCL rather than the fold kernel */
int psp_csr_multi_info(const psp_csr_t *A, int *nranks, int *distinct_devices, int *uses_rccl);
/* The partition psp_csr_create_multi computes for rank `rank` of `ndev`, as pure host code (no device needed: the CPU tests
 * compare it with general_halo_plan of pysparse_amd/distributed.py): row_range_out = {row_lo, row_hi}; counts_out =
 * {ghost_lo, ghost_hi, interior_a, interior_b, nlinks}; ghost_ids (may be NULL) = the sorted global ids of the ghost entries;
 * links (may be NULL) = nlinks x {sending rank, offset in the extended vector, count, send offset in the sender's owned
 * entries or -1 for a gathered index list}; col_local (may be NULL, ind[row_hi] - ind[row_lo] ints) = the block's columns in
 * [ghost_lo | owned | ghost_hi] numbering. */
int psp_multi_plan(int nrows, int ncols, const int *ind_host, const int *col_host, int ndev, int rank,
                   int64_t *row_range_out, int *counts_out, int *ghost_ids, int ghost_cap, int *links, int links_cap,
                   int *col_local);
/* timing hook: `reps` products y = A x on resident slices, each done the way a solver iteration does it (ghost
 * copies on the copy streams, the rows that need none meanwhile, then the boundary rows); *ms_per_product is the
 * slowest rank's stream time per product (HIP events on every rank's compute stream) */
int psp_csr_multi_spmv_time(psp_csr_t *A, int warmup, int reps, double *ms_per_product);
/* the pieces of that product and of an iteration on their own, same timing: what 0 = the ghost exchange alone,
 * 1 = the local product alone (no exchange), 2 = one packed reduction of two doubles (RCCL all-reduce or the fold
 * kernel).  bench.py reports them as `phases` of the single-process line; the halo time hidden behind the interior
 * rows is (t0 + t1 - t_product) / t0. */
int psp_csr_multi_phase_time(psp_csr_t *A, int what, int warmup, int reps, double *ms_per_rep);
/* General CSR beyond the reference's C int (csr_mat.h:6-13: `int nnz`, `int *ind`): row offsets are 64-bit at
 * this boundary, column indices stay 32-bit.  Above 2^30 nonzeros the rows are cut into parts of < 2^30
 * nonzeros that share x and write disjoint row ranges of y ("64-bit row offsets ... or
 * partitions resident on one device"): the SpMV kernels never see a 64-bit offset.  matvec, the diagonal,
 * jacobi and the solvers work on such a handle; download goes by row ranges; there is no transposed product. */
int psp_csr_create64(int nrows, int ncols, int64_t nnz, const int64_t *ind_host, const int *col_host,
                     const double *val_host, psp_csr_t **out);
/* Synthetic general (non-stencil) CSR generated on the device, for tests and measurements at sizes no host
 * array reaches: row r stores m entries, entry j in column (r + (j - m/2)*stride + h(r, j) mod stride) mod ncols
 * with a value in [-1, 1), h = splitmix64 of (seed, r, j) (psp_csr.hip: random_banded_kernel; the tests restate
 * the formula).  nrows*m may exceed 2^31. */
int psp_csr_random_banded(int nrows, int ncols, int m, int stride, uint64_t seed, psp_csr_t **out);
/* rows [row_lo, row_hi) of any handle with CSR arrays: ind_host gets row_hi - row_lo + 1 offsets relative to
 * row_lo; col_host / val_host (may be NULL) the entries */
int psp_csr_download_rows(const psp_csr_t *A, int row_lo, int row_hi, int64_t *ind_host, int *col_host,
                          double *val_host);
int psp_csr_destroy(psp_csr_t *A);
/* shape / nnz attributes: CSRMatType_getattr, csr_mat.c:208-231 */
int psp_csr_shape(const psp_csr_t *A, int *nrows, int *ncols, int *nnz);
/* copy the device arrays back (structure parity tests; any pointer may be NULL) */
int psp_csr_download(const psp_csr_t *A, int *ind_host, int *col_host, double *val_host);
/* A[i,i] for all rows (0.0 where no diagonal entry is stored) */
int psp_csr_diagonal(const psp_csr_t *A, double *diag_host);

/* y := A x.  CSRMat_matvec, csr_mat.c:141-163 (kernel :49-54); x has ncols, y nrows
 * entries; y is overwritten.  Per-row summation is left to right from 0.0 with separate
 * multiply and add, so results are bit-identical to the reference loop. */
int psp_csr_matvec(psp_csr_t *A, const double *x_host, double *y_host);
/* element strides of non-contiguous NumPy views: csr_matvec_kernel_stride, csr_mat.c:58-72 */
int psp_csr_matvec_stride(psp_csr_t *A, const double *x_host, ptrdiff_t incx, double *y_host,
                          ptrdiff_t incy);
/* y := A^T x.  CSRMat_matvec_transp, csr_mat.c:114-133 (kernel :74-88).  Every y[c] adds its terms by
 * ascending row like the reference's scatter loop, so the result is bit-identical: offset-structured
 * matrices gather over the w4 layout, all others multiply with A^T kept as a second CSR matrix (built
 * on the first call, + one matrix of device memory). */
int psp_csr_matvec_transp(psp_csr_t *A, const double *x_host, double *y_host);
int psp_csr_matvec_transp_stride(psp_csr_t *A, const double *x_host, ptrdiff_t incx,
                                 double *y_host, ptrdiff_t incy);
/* device-pointer flavours (no synchronisation) */
int psp_csr_matvec_dev(psp_csr_t *A, const double *x_dev, double *y_dev);
int psp_csr_matvec_transp_dev(psp_csr_t *A, const double *x_dev, double *y_dev);
/* kernel tuning knob for A/B measurements: variant < 0 restores the default */
int psp_csr_set_variant(psp_csr_t *A, int variant);
/* workgroup schedule of the SpMV (tuning / tests; results never depend on it): strip_rows < 0
 * automatic (plane-sweeping order for wide-band operators such as the 7-point stencil), 0 natural
 * row order, > 0 plane-sweeping with that many rows per strip regardless of the matrix size */
int psp_csr_set_schedule(psp_csr_t *A, int strip_rows);
/* which kernel y := A x runs for this handle (builds its tables if needed): name, and
 * info[4] = {w3: x blocks per chunk list / w4: number of distinct col-row offsets,
 * most x blocks one chunk references (w3), schedule active, half band width used by the schedule}.
 * csr_spmv_w4: offset-structured operators (<= 32 distinct col - row, ascending columns), values in
 *   offset-major blocks + 16-bit row masks; csr_spmv_w3: banded CSR, x staged in LDS, 16-bit
 *   chunk-local columns; csr_spmv_w2 / w1 / stream: any CSR.  All add each row's products left
 *   to right (csr_mat.c:49-54), so the choice never changes a bit of y. */
int psp_csr_kernel_info(psp_csr_t *A, char *name, int name_cap, int *info);
/* Set-up against steady state for irregular numberings (round 6; no reference analogue: csr_mat.c:259-296 builds nothing).
 * A csr_mat whose stored numbering scatters its columns (an FEM mesh as it comes out of a generator) multiplies 4-12 us
 * faster per product, and iterates 16-24 us faster per Jacobi-MINRES iteration, through a renumbered copy (reverse
 * Cuthill-McKee, "csr_spmv_w3_rcm") than on the stored numbering ("csr_spmv_w5") -- and the copy costs 17-57 ms to build at
 * n = 9.3e5.  The library therefore builds it only once a handle has done 2048 products (solver iterations included), or at
 * the next product after the caller has announced at least that many here.  y = A x has the same bits either way; a fused solve's iterates differ at rounding level between the two
 * numberings (its dot products add in the numbering it runs in), deterministically for a given sequence of calls.
 * psp_csr_setup_info: info4 = {ms the copy took to build (0: not built), products counted so far, the threshold,
 * state (-1 undecided, 0 examined and not built, 1 built)}. */
int psp_csr_prepare(psp_csr_t *A, long long expected_products);
/* An offset-structured csr_mat (csr_spmv_w4, <= 16 distinct col - row) multiplies with its index-free tables; the CSR arrays
 * it was created from stay for download, the variants and ABI parity with CSRMatObject (csr_mat.h:6-13) -- 1.65 x the
 * memory (512^3: 11.8 GB of arrays beside 7.8 GB of tables).  A caller that needs neither frees them here: the handle then
 * supports matvec (incl. the transposed product), diagonal / jacobi, the solvers and kernel_info, like the operator of
 * psp_csr_poisson_big; psp_csr_download fails with PSP_EINVAL and psp_csr_set_variant has nothing left to select.  Results do not change by a bit.
 * PSP_EINVAL for handles that stream their CSR arrays (w3 / w6 / w2 / w5). */
int psp_csr_release_arrays(psp_csr_t *A);
int psp_csr_setup_info(psp_csr_t *A, double *info4);
/* The renumbering behind "csr_spmv_w3_rcm" (irregular square operators): perm_host[new] = old row
 * (nrows ints) and *available = 2 (numbering computed on the device) or 1 (on the host: fallback, A/B switch) when
 * psp_csr_kernel_info / a product has built one for this handle; *available = 0 otherwise (perm_host untouched).
 * Diagnostic: no product needs it. */
int psp_csr_renumbering(psp_csr_t *A, int *perm_host, int *available);
/* bytes of device memory held by the handle */
int64_t psp_csr_device_bytes(const psp_csr_t *A);

/* ------------------------------------------------------------------ sss_mat */

/* replaces newSSSMatObject + LLMat_to_sss (sss_mat.c:243-284, ll_mat.c:1654-1708):
 * strict lower triangle in CSR form (nnz_lower entries) + dense diagonal. */
int psp_sss_create(int n, int nnz_lower, const int *ind_host, const int *col_host,
                   const double *val_host, const double *diag_host, psp_sss_t **out);
/* symmetric-skyline form of the Poisson operator (poisson2d_sym(n).to_sss()) */
int psp_sss_poisson(int nx, int ny, int nz, psp_sss_t **out);
int psp_sss_destroy(psp_sss_t *A);
/* n, and nnz as the reference reports it: strict-lower count + n (sss_mat.c:155) */
/* which kernel y := S x runs (sss_spmv_w4 for offset-structured matrices: the strict lower triangle
 * only, half the traffic of the mirrored product; otherwise the csr kernels on the full mirror),
 * and the A/B knob -- same meaning as psp_csr_kernel_info / psp_csr_set_variant */
int psp_sss_kernel_info(psp_sss_t *A, char *name, int name_cap, int *info);
/* psp_csr_prepare / psp_csr_setup_info for the mirror an irregular sss_mat multiplies with */
int psp_sss_prepare(psp_sss_t *A, long long expected_products);
int psp_sss_setup_info(psp_sss_t *A, double *info4);
int psp_sss_set_variant(psp_sss_t *A, int variant);
int psp_sss_shape(const psp_sss_t *A, int *n, int *nnz_reported);
int psp_sss_download(const psp_sss_t *A, int *ind_host, int *col_host, double *val_host,
                     double *diag_host);
/* A[i,j]: getitem, sss_mat.c:14-28 */
int psp_sss_getitem(const psp_sss_t *A, int i, int j, double *value);
/* y := A x (== A^T x).  SSSMat_matvec, sss_mat.c:78-96 (kernel :40-56).  Per row the
 * terms are added in the reference's order: lower entries by ascending column, the
 * diagonal term, then the mirrored upper entries by ascending row. */
int psp_sss_matvec(psp_sss_t *A, const double *x_host, double *y_host);
int psp_sss_matvec_stride(psp_sss_t *A, const double *x_host, ptrdiff_t incx, double *y_host,
                          ptrdiff_t incy);
int psp_sss_matvec_dev(psp_sss_t *A, const double *x_dev, double *y_dev);
int64_t psp_sss_device_bytes(const psp_sss_t *A);

/* ------------------------------------------------------------------- jacobi */

/* replaces newJacobiObject (pysparse/precon/src/preconmodule.c:352-412):
 * dinv[i] = omega / A[i,i]; PSP_ESINGULAR if 1.0 + A[i,i] == 1.0 for some i (:395).
 * The native forms read the diagonal on the device instead of n calls of A[i,i].
 * steps > 1 keeps a reference to the operator for the extra sweeps (:45-52). */
int psp_jacobi_create_csr(psp_csr_t *A, double omega, int steps, psp_jacobi_t **out);
int psp_jacobi_create_sss(psp_sss_t *A, double omega, int steps, psp_jacobi_t **out);
/* generic form: host diagonal (already fetched through A[i,i]) + the operator used by
 * the steps > 1 sweeps (may be NULL when steps == 1) */
int psp_jacobi_create_diag(int n, const double *diag_host, double omega, int steps,
                           const psp_op_t *A_or_null, psp_jacobi_t **out);
int psp_jacobi_destroy(psp_jacobi_t *K);
int psp_jacobi_shape(const psp_jacobi_t *K, int *n);
/* y := K x.  Jacobi_precon, preconmodule.c:60-80 (kernel :35-54) */
int psp_jacobi_precon(psp_jacobi_t *K, const double *x_host, double *y_host);
int psp_jacobi_precon_dev(psp_jacobi_t *K, const double *x_dev, double *y_dev);

/* --------------------------------------------------------------------- ssor */

/* replaces newSSORObject (preconmodule.c:414-459): `steps` symmetric Gauss-Seidel (omega == 1,
 * symgs_kernel :149-193) or SSOR (ssor_kernel :95-143) steps with a zero initial guess on an
 * sss_mat.  The triangular sweeps are level-scheduled; every row performs the reference's
 * operations in the reference's order, so results are bit-identical to the sequential loops.
 * The handle borrows A (keep it alive). */
int psp_ssor_create(psp_sss_t *A, double omega, int steps, psp_ssor_t **out);
int psp_ssor_destroy(psp_ssor_t *K);
/* n and the number of dependency levels of the forward / backward sweep */
int psp_ssor_info(const psp_ssor_t *K, int *n, int *levels_forward, int *levels_backward);
/* how much of the schedule runs as single-workgroup runs of narrow levels that exchange x through LDS (2-D operators,
 * the thin ends of 3-D ones) instead of one launch per level: runs per direction, levels and slots covered; no
 * reference analogue (the reference's sweeps are sequential, preconmodule.c:95-193) */
int psp_ssor_run_info(const psp_ssor_t *K, int *runs_forward, int *runs_backward, long *levels_in_runs,
                      long *slots_in_runs);
/* 3-D grid operators whose levels are too wide for such runs are swept brick by brick (bricks of `edge`^3 grid points, a
 * coarse wavefront of workgroups): the number of bricks, 0 when the handle does not use them */
int psp_ssor_brick_info(const psp_ssor_t *K, int *bricks, int *edge);
/* y := K x.  SSOR_precon, preconmodule.c:199-223 */
int psp_ssor_precon(psp_ssor_t *K, const double *x_host, double *y_host);
int psp_ssor_precon_dev(psp_ssor_t *K, const double *x_dev, double *y_dev);

/* ---------------------------------------------------------------- multigrid */

/* precon.multigrid(A, grid, omega, steps): a geometric V-cycle for A = sum_a c_a T_a + s I on a grid of 1 to 3 axes
 * (T_a = [-1 2 -1] along axis a, nothing stored across line ends, row k = i0 + n0 i1 + n0 n1 i2), matrix-free: c_a and
 * s are read from A at creation, where a device pass checks that EVERY stored entry is the stencil's (PSP_EINVAL
 * otherwise, also for a multi-device matrix); A is not used afterwards.  Axes with n_a >= 4 are halved level by level
 * (coarse point j at fine 2j + 1, c_a / 4), `steps` damped-Jacobi sweeps before and after, a dense solve on the coarsest
 * level (at most 27 points); 0 < omega <= 1, steps >= 1: the operator is symmetric positive definite.  DESIGN.md 9c.
 * No reference analogue (the reference's preconditioners are jacobi and ssor); no host mode. */
int psp_mg_create_csr(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out);
int psp_mg_create_sss(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out);
int psp_mg_destroy(psp_mg_t *K);
/* y := K x (y must not alias x in the device form); same bits from call to call */
int psp_mg_precon(psp_mg_t *K, const double *x_host, double *y_host);
int psp_mg_precon_dev(psp_mg_t *K, const double *x_dev, double *y_dev);
/* levels, the first level of the single-workgroup tail launch (that level and all below it run in one kernel with their
 * vectors in LDS), kernel launches per application, and the level dimensions (3 ints per level, 1 on absent axes;
 * dims may be NULL) */
int psp_mg_info(const psp_mg_t *K, int *levels, int *tail_first_level, int *launches_per_apply, int *dims);
/* Y[:, c] := K X[:, c] for c < k in ONE block cycle (either mode): column-major blocks, column c at X + c*ldx and
 * Y + c*ldy, ldx, ldy >= n, k >= 1; Y must not overlap X (PSP_EINVAL).  Column c has the bits of psp_mg_precon on that
 * column; the cycle is launches_per_apply launches whatever k is, and the level operators of a Galerkin handle are
 * streamed once per group of columns instead of once per column.  PSP_ENODEV with PSP_DEVICE=cpu. */
int psp_mg_precon_block(psp_mg_t *K, int k, const double *X_host, long ldx, double *Y_host, long ldy);
int psp_mg_precon_block_dev(psp_mg_t *K, int k, const double *X_dev, long ldx, double *Y_dev, long ldy);
/* The block cycle's level vectors: a second set on the handle, about (1 + 3/7) n 8 k bytes on a 3-D grid, allocated by
 * the first block call for its k and grown on demand.  psp_mg_block_reserve allocates them ahead of time for at least k
 * columns (k = 0 frees them); psp_mg_block_info reports the columns they hold and their bytes (either may be NULL).
 * psp_mg_destroy frees them, psp_trim does not touch them. */
int psp_mg_block_reserve(psp_mg_t *K, int k);
int psp_mg_block_info(psp_mg_t *K, int *columns, long long *bytes);

/* precon.multigrid(A, grid, omega, steps, galerkin=True): the same cycle (level grids, P, R, smoother, tail, dense
 * coarsest solve) for ANY symmetric 3- / 5- / 7-point operator on the grid, e.g. -div(kappa grad u) + s u with kappa varying
 * from cell to cell: the level operators are A_0 = A, A_{l+1} = R_l A_l P_l, stored as symmetric stencils (the diagonal
 * and one array per lower offset), the smoother is x += (omega / diag(A_l)) o (b - A_l x).  DESIGN.md 9d.  One device pass
 * checks every row: entries only at offset 0 or +-stride of an axis with n_a > 1, none across a line end, none twice, the
 * diagonal stored, finite and > 0, A[k, k+st] == A[k+st, k] bit for bit (a neighbour that is not stored counts as 0);
 * anything else is PSP_EINVAL naming the first kind of violation, as are multi-device handles, handles stored in parts
 * and handles without their index arrays (psp_csr_poisson_big, after psp_csr_release_arrays).  PSP_ESINGULAR when a level
 * diagonal is not finite and > 0.  The handle is used through psp_mg_precon / _precon_dev / _info / _destroy and
 * psp_op_from_mg like the matrix-free one. */
int psp_mg_create_csr_galerkin(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out);
int psp_mg_create_sss_galerkin(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out);
/* 1 when the handle stores Galerkin level operators, 0 for the matrix-free mode */
int psp_mg_is_galerkin(const psp_mg_t *K, int *galerkin);
/* Test hook: level `level`'s stored stencil arrays, the diagonal first, then one array per lower offset o with entry K =
 * A_l[K, K+o] (0 where that neighbour does not exist); every level, those of the tail included.  *noff_inout: in, the
 * room in arrays; out, the arrays of the level (1 + lower offsets).  offsets_out takes 3 ints (d0, d1, d2) per array,
 * values_host prod(level grid) doubles per array; with both NULL only the count is returned.  PSP_EINVAL for a
 * matrix-free handle. */
int psp_mg_level_operator(psp_mg_t *K, int level, int *offsets_out, int *noff_inout, double *values_host);

/* The general creation call: flags = 0 is psp_mg_create_csr / _sss, PSP_MG_GALERKIN the _galerkin pair (the four are
 * calls of these), PSP_MG_SINGLE the single-precision cycle of either mode (precision='single'); any
 * other bit is PSP_EINVAL.  The single-precision cycle is the mode's cycle evaluated in IEEE float32 on rounded data: the
 * level operators (c_a, d, omega / d; the Galerkin chain and omega / diagonal) and the coarsest inverse are formed in
 * double exactly as without the flag, then every stored number is rounded once to float; b is rounded as it is read,
 * every sweep, restriction, prolongation and the tail run in float in the same summation orders, and the result is
 * widened into y.  x and y stay double vectors: the handle is used like any other (psp_mg_precon*, psp_op_from_mg, the
 * solvers), with the same level grids and launches, the same bits from call to call, from host and device entry
 * points, from csr and sss handles and from column c of a block.  PSP_EINVAL naming the single-precision range when a
 * level diagonal or omega / diagonal is not finite, not > 0 or below FLT_MIN after rounding; the same matrix is
 * accepted without the flag.  A Galerkin handle releases each level's double arrays as soon as the next level is built:
 * at rest it holds float arrays only. */
#define PSP_MG_GALERKIN 1u
#define PSP_MG_SINGLE 2u
int psp_mg_create_csr_ex(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, unsigned flags, psp_mg_t **out);
int psp_mg_create_sss_ex(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, unsigned flags, psp_mg_t **out);
/* 64, or 32 for a handle created with PSP_MG_SINGLE */
int psp_mg_precision(const psp_mg_t *K, int *bits);
/* What the handle holds on the device at rest, the block cycle's vectors (psp_mg_block_info) excluded: the level
 * operators with the coarsest inverse and the tail's table, and the level vectors.  Either pointer may be NULL.
 * psp_mg_level_operator on a single-precision handle returns the stored floats widened to double. */
int psp_mg_bytes(const psp_mg_t *K, long long *operator_bytes, long long *vector_bytes);

/* precon.multigrid(A, grid, omega, steps, galerkin=True, line=a): the Galerkin cycle with a line smoother, for grids
 * whose cells are graded or stretched along axis a.  The accepted operators, the checking pass and its
 * refusals are psp_mg_create_*_galerkin's.  Axis a is never coarsened; every other axis is halved while it has at least 2
 * points (n' = n / 2; 3 -> 1 and 2 -> 1 included), so that the last level is the single line (1, .., n_a, .., 1).  The
 * smoother is x += omega T_l^-1 (b - A_l x) with T_l the diagonal of A_l and its entries at offset -+stride_a: one
 * tridiagonal solve per grid line, factorised once per level at creation (p_0 = d_0, p_i = d_i - l_i (l_i / p_{i-1}); 1 / p
 * is stored where the point smoother stores omega / diagonal).  The last level is solved exactly by one such solve.  There
 * is no tail kernel and no dense inverse: psp_mg_info reports tail_first_level == levels and
 * launches_per_apply = (levels - 1)(2 steps + 2) + 1.  Symmetric positive definite for 0 < omega <= 1; no atomics, the
 * same bits from call to call, from csr and sss handles and from host and device entry points.
 * PSP_EINVAL (before any device call) for ndim == 1, line_axis outside 0 .. ndim - 1 and a line axis of fewer than 2
 * points; PSP_ESINGULAR when a pivot p_i is not finite and > 0.  There is no single-precision form.  The handle is used
 * like any other (psp_mg_precon*, psp_op_from_mg, psp_mg_level_operator, _bytes, _info, _destroy); psp_mg_precon_block*
 * applies the single cycle column by column (column c has the bits of psp_mg_precon, psp_mg_block_info reports 0
 * columns and psp_mg_block_reserve does nothing). */
int psp_mg_create_csr_line(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, int line_axis, psp_mg_t **out);
int psp_mg_create_sss_line(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, int line_axis, psp_mg_t **out);
/* the line axis of a handle created by psp_mg_create_*_line, -1 for every other handle */
int psp_mg_line_axis(const psp_mg_t *K, int *axis);

/* precon.multigrid(A, grid, omega, steps, galerkin=True, stencil='box'): the Galerkin cycle for symmetric operators with the
 * full pattern {-1, 0, 1}^ndim -- 9 points in 2-D, 27 in 3-D (Q1 finite elements, the compact 9-point Laplacian, -div(kappa
 * grad u) with kappa per cell); DESIGN.md 9i.  A flag of psp_mg_create_csr_ex / _sss_ex, valid only together with
 * PSP_MG_GALERKIN (PSP_EINVAL without it); PSP_MG_SINGLE may be added.  Row r and column c are split into grid coordinates
 * (r = r0 + n0 r1 + n0 n1 r2): an entry is accepted iff c_a - r_a lies in {-1, 0, 1} on every axis, so an entry that wraps
 * across a line end is an offset violation and an axis of length 1 never carries a difference.  As for the axis pattern no
 * entry may be stored twice, the diagonal is stored, finite and > 0, and A[r, c] has the bits of A[c, r] (a neighbour that
 * is not stored counts as +0.0); PSP_EINVAL names the first kind in the order offset, duplicate, diagonal, symmetry.  Level 0
 * is stored in the layout of every lower level: the diagonal, omega / diagonal and all (3^ndim - 1) / 2 lower arrays (15
 * arrays per point in 3-D against 5 of an axis handle), and the cycle's kernels take it as they take the lower levels; the
 * level grids, transfers, tail, dense coarsest solve, launches and determinism are PSP_MG_GALERKIN's.  The Galerkin products
 * of a handle of 2 or 3 axes sum the same terms in the same order as PSP_MG_GALERKIN's but keep the rounding errors of the
 * running sum and add them at the end (each entry is the exact sum rounded to within an ulp or two).  In 1-D the two
 * patterns coincide and the handle has the bits of the axis one.  There is no line-smoothed form. */
#define PSP_MG_BOX 8u /* bit 2 (4u) stays unassigned and is refused like every unknown bit */
/* *box = 1 for a handle created with PSP_MG_BOX, 0 for every other handle */
int psp_mg_stencil(const psp_mg_t *K, int *box);

/* precon.multigrid(A, grid, omega, steps, galerkin=True, interp='operator'): the Galerkin cycle with operator-dependent
 * ("black box") interpolation, for coefficients that jump between regions a few cells wide; DESIGN.md 9j.  A flag of
 * psp_mg_create_csr_ex / _sss_ex, valid only together with PSP_MG_GALERKIN; PSP_MG_BOX may be added, PSP_MG_SINGLE may not
 * (PSP_EINVAL, "not supported", before any device call), and psp_mg_create_*_line has no such form.  The accepted
 * operators, the checking pass, the level grids and the smoother are those of the handle without the flag.  The
 * prolongation of level l is derived from the level's stored stencil S_p[d]: along a coarsened axis an odd fine index has
 * the single parent (i - 1) / 2, an even one lies between its parents i / 2 - 1 and i / 2; with F the axes on which point p
 * lies between, the stencil is collapsed onto F (T[delta] = sum of S_p[d] over the d that agree with delta on F) and
 * w_p = -sum over delta != 0 of (T[delta] / T[0]) w_{p + delta}, neighbours inside the grid only, in rounds |F| = 1, 2, 3; a
 * point whose T[0] is not finite and > 0 takes the linear weights and is counted.  R = P' / 2^(coarsened axes),
 * A_{l+1} = R A_l P with the two-sum accumulation of PSP_MG_BOX.  Restriction and prolongation are gathers without atomics:
 * the same bits from call to call, from csr and sss handles and from host and device entry points.  There is no tail
 * kernel: every level above the last is launches, the dense product of the last level is one more; psp_mg_info reports
 * tail_first_level == levels and launches_per_apply = (levels - 1)(max(steps - 1, 1) + steps + 2) + 1.  psp_mg_precon_block*
 * applies the single cycle column by column (psp_mg_block_info reports 0 columns, psp_mg_block_reserve does nothing).
 * psp_mg_bytes counts the weights as operator bytes. */
#define PSP_MG_INTERP 16u
/* *operator_dependent = 1 for a handle created with PSP_MG_INTERP, 0 for every other handle */
int psp_mg_interp(const psp_mg_t *K, int *operator_dependent);
/* the points of level `level` (0 .. levels - 2) that took the linear weights; PSP_EINVAL without PSP_MG_INTERP */
int psp_mg_interp_fallbacks(psp_mg_t *K, int level, long long *points);
/* Test hook: the weights of the prolongation from level `level` + 1 to `level` (0 .. levels - 2), slot-major over the
 * level's fine points: slot s, point p at W_host[s * prod(level grid) + p].  There are 2^ndim slots, of which those with a
 * bit on an axis that is not coarsened hold zeros.  Bit a of s names the parent along axis a: 0 the lower one -- coarse
 * index i_a / 2 - 1 of an even fine index i_a, the only parent (i_a - 1) / 2 of an odd one, i_a itself on an axis that is
 * not coarsened --, 1 the upper one, coarse index i_a / 2 of an even fine index.  A slot whose parent does not exist
 * holds 0.  *nslots_inout: in, the room in slots; out, 2^ndim; with W_host NULL only the count is returned. */
int psp_mg_transfer_weights(psp_mg_t *K, int level, int *nslots_inout, double *W_host);

/* --------------------------------------------------------- operator protocol */

/* Host callback operator: the C image of SpMatrix_Matvec / SpMatrix_Precon
 * (spmatrixmodule.c:169-201, :215-248).  Called with HOST vectors; returns 0, or
 * non-zero when the callee failed (a Python exception is pending). */
typedef int (*psp_host_apply_fn)(void *ctx, int n, const double *x_host, double *y_host);

int psp_op_from_csr(psp_csr_t *A, psp_op_t **out);
int psp_op_from_sss(psp_sss_t *A, psp_op_t **out);
int psp_op_from_jacobi(psp_jacobi_t *K, psp_op_t **out);
int psp_op_from_ssor(psp_ssor_t *K, psp_op_t **out);
int psp_op_from_mg(psp_mg_t *K, psp_op_t **out);
int psp_op_from_callback(int n, psp_host_apply_fn fn, void *ctx, psp_op_t **out);
int psp_op_destroy(psp_op_t *op);

/* ------------------------------------------------------------------ solvers */

/* info, iter, relres = pcg(A, b, x, tol, maxit[, K]) -- ItSolvers_pcg
 * (itsolversmodule.c:32-118) + Itsolvers_pcg_kernel (pysparse/itsolvers/src/pcg.c:22-171).
 * The whole loop runs on the device; b and x cross PCIe once each way.  Semantics kept:
 * tolb = tol*||b||; b == 0 -> x := 0, info 0; iter == maxit+1 when not converged;
 * stagnation / breakdown codes as above.  K may be NULL.  hist_host (may be NULL, maxit+1
 * doubles) receives ||r|| per iteration.  Returns PSP_ECALLBACK when a callback failed
 * (the reference returns -1 from the kernel, pcg.c:8-11). */
int psp_pcg(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
            double tol, int maxit, int *info, int *iter, double *relres, double *hist_host);
int psp_pcg_dev(const psp_op_t *A, const psp_op_t *K, int n, double *x_dev, const double *b_dev,
                double tol, int maxit, int *info, int *iter, double *relres, double *hist_host);

/* info, iter, relres = minres(A, b, x, tol, maxit[, K]) -- ItSolvers_minres
 * (itsolversmodule.c:217-305) + Itsolvers_minres_kernel (pysparse/itsolvers/src/minres.c:43-200).
 * *relres is written only on the 0 / -1 exits, as in the reference. */
int psp_minres(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
               double tol, int maxit, int *info, int *iter, double *relres, double *hist_host);
int psp_minres_dev(const psp_op_t *A, const psp_op_t *K, int n, double *x_dev,
                   const double *b_dev, double tol, int maxit, int *info, int *iter,
                   double *relres, double *hist_host);

/* The four other Krylov kernels of the reference's `krylov` module on the same operator
 * protocol, unfused: cgs (pysparse/itsolvers/src/cgs.c:14-110,
 * wrapper itsolversmodule.c:503-586), bicgstab (bicgstab.c:233-320, :125-216), qmrs
 * (qmrs.c:29-154, :410-496; the initial guess is ignored), gmres(dim)
 * (gmres.c:62-175, :313-403; *relres is the true residual reduction). */
int psp_cgs(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
            double tol, int maxit, int *info, int *iter, double *relres);
int psp_bicgstab(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
                 double tol, int maxit, int *info, int *iter, double *relres);
int psp_qmrs(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
             double tol, int maxit, int *info, int *iter, double *relres);
int psp_gmres(const psp_op_t *A, const psp_op_t *K, int n, double *x_host, const double *b_host,
              double tol, int maxit, int dim, int *info, int *iter, double *relres);

/* ------------------------------------------------------------------ block vectors
 * Tall-skinny dense algebra on n x m blocks (m a few dozen columns): what the Jacobi-Davidson eigensolver does besides
 * its products -- the dgemv / dgemm calls of jdsym.c:265-266, :334, :366-371, :416-421, :508-513, :607-608, orthopack.c:56-57
 * and correq.c:61-63, :82-90.  Column c of a block starts at V_dev + c*ld, ld >= n; rows n..ld of a column are never read
 * or written.  All three enqueue on the calling thread's stream and return without synchronising.
 *   tdot   : h[c] = sum_i V[i,c] x[i], c < m.  Fixed-order partial sums, no atomics: two runs give identical bits.
 *            Streams 8 n (m + 1) bytes (x once per group of eight columns).
 *   gemv   : y[i] = beta y[i] + alpha sum_c V[i,c] h[c], terms added for c ascending; h on the device; beta == 0 does not
 *            read y.  q = V u (alpha 1, beta 0) and x -= V h (alpha -1, beta 1) are this one kernel.
 *   rotate : V[:, dst0 .. dst0+jn) = V[:, 0 .. j) U[:, u0 .. u0+jn) in place, U (j x j, column-major, leading dimension
 *            ldu) on the host; every row is read completely before its results are written, so the ranges may overlap.
 *            j <= 128. */
int psp_bv_tdot(int n, int m, const double *V_dev, int64_t ld, const double *x_dev, double *h_dev);
int psp_bv_gemv(int n, int m, const double *V_dev, int64_t ld, const double *h_dev, double alpha, double beta,
                double *y_dev);
int psp_bv_rotate(int n, int j, double *V_dev, int64_t ld, const double *U_host, int ldu, int u0, int jn, int dst0);
/* The block kernels of psp_lobpcg, same layout rules.
 *   gram  : G[a + b ldg] = sum_i A[i,a] B[i,b] (ma x mb entries, nothing else of G is written), a thread keeping an
 *           8 x 4 tile of sums, so A is streamed ceil(mb / 4) times and B ceil(ma / 8) times.  Column b of G has the bits
 *           of psp_bv_tdot(n, ma, A, lda, B + b ldb, h) whenever both take the same access form: the 16-byte form iff n,
 *           lda and ldb are even and both bases are 16-byte aligned (tdot alternates from column to column when ldb is
 *           odd and n even: those columns agree to rounding only).  With A == B, G is exactly symmetric.
 *   resid : for c < k (k <= 32): r = AX[:,c] - theta[c] MX[:,c] (the product rounded, then the difference), written to
 *           R[:, slot[c]] where slot[c] >= 0 (slot_host: k ints on the host, distinct where >= 0 and < k) and nowhere
 *           otherwise; nrm2[c] = r . r for every c with the bits of psp_bv_tdot(n, 1, R_c, ldr, R_c, h) on the stored
 *           column.  MX_dev may be the X block itself; R must not overlap AX or MX. */
int psp_bv_gram(int n, int ma, const double *A_dev, int64_t lda, int mb, const double *B_dev, int64_t ldb, double *G_dev,
                int64_t ldg);
int psp_bv_resid(int n, int k, const double *AX_dev, int64_t ldax, const double *MX_dev, int64_t ldmx,
                 const double *theta_dev, const int *slot_host, double *R_dev, int64_t ldr, double *nrm2_dev);

/* ------------------------------------------------------------------ psp_lobpcg: block eigensolver (psp_lobpcg.hip)
 * The k smallest eigenpairs of A x = lambda M x by LOBPCG: A symmetric, M symmetric positive definite or NULL (identity),
 * K a symmetric positive definite preconditioner for A or NULL; 1 <= k <= 32, 3 k <= n.  Every n-vector stays on the
 * device; per iteration K is applied ONCE to the block of active residuals (psp_op_apply_block_dev: one block V-cycle for a
 * multigrid handle) and A (and M) multiply ONE block.  X0_host: x0_cols (0 .. k) start columns, column-major with leading
 * dimension ldx0; the other columns come from the device generator of psp_jdsym.  A column with ||A x - theta M x||_2 <=
 * tol (x M-normalised; absolute, like jdtol) is soft-locked.  When every column passes, A X and M X are recomputed by
 * explicit products and the test is repeated on them before the call returns.
 * On return: lambda_host[k] ascending, X_host (n x k, column-major, leading dimension ldx) M-orthonormal, res_host[k] the
 * explicit residual norms, *kconv the columns with res <= tol, *it the iterations done (itmax reached is not an error).
 * psp_last_solve_info names the loop "lobpcg"; its info[2] is the number of restarts (Rayleigh-Ritz steps repeated without
 * P because S' M S did not factor), info[0] and info[1] are -1.
 * PSP_EINVAL: k or n out of range, tol <= 0, itmax < 0, operators of different order, multi-device or split operands --
 * all before any device call; PSP_ENODEV with PSP_DEVICE=cpu. */
int psp_lobpcg(const psp_op_t *A, const psp_op_t *M, const psp_op_t *K, int n, int k, double tol, int itmax,
               const double *X0_host, int x0_cols, long ldx0, double *lambda_host, double *X_host, long ldx,
               double *res_host, int *kconv, int *it);
/* Test hook of its projected problem (no device needed): GA c = lambda GM c of order m <= 128, both matrices column-major
 * with leading dimension ld and symmetrised on entry; lambda_host ascending, C_host (m x m, leading dimension ld) with
 * C' GM C = I and C' GA C = diag(lambda).  PSP_ESINGULAR when GM is not positive definite. */
int psp_debug_gen_ritz(int m, const double *GA_host, const double *GM_host, int ld, double *lambda_host, double *C_host);

/* ------------------------------------------------------------------ products and PCG on blocks of vectors
 * Y[:, c] = A X[:, c] for c < k with the matrix streamed once per group of up to eight columns (psp_spmm.hip).  Blocks
 * are column-major like the psp_bv_* ones: column c of X starts at X + c*ldx (ldx >= ncols), column c of Y at
 * Y + c*ldy (ldy >= nrows); rows beyond the matrix order and columns >= k are never written.  Column c has the BITS of
 * psp_csr_matvec / psp_sss_matvec on X[:, c] (every kernel adds a row's products left to right).  Handles whose product
 * is csr_spmv_w4 (<= 9 offsets; psp_csr_poisson_big and psp_csr_release_arrays handles included) run the index-free block
 * kernel csr_spmm_w4, every other handle that still has its CSR arrays runs csr_spmm_rows; an sss_mat multiplies through
 * its expanded mirror.  PSP_EINVAL: a multi-device matrix, a matrix stored in parts, a released handle with more than 9
 * offsets, X and Y overlapping, k < 1, a leading dimension below the vector length.  PSP_DEVICE=cpu: PSP_ENODEV.
 * The *_dev forms enqueue on the calling thread's stream and return without synchronising.
 * psp_op_apply_block_dev: the same for any operator -- csr / sss as above, jacobi with steps = 1 one scaling kernel, a
 * multigrid handle one block cycle (psp_mg_precon_block_dev), every other kind (ssor, host callback, jacobi with more
 * steps) column by column. */
int psp_csr_matmat(psp_csr_t *A, int k, const double *X_host, long ldx, double *Y_host, long ldy);
int psp_csr_matmat_dev(psp_csr_t *A, int k, const double *X_dev, long ldx, double *Y_dev, long ldy);
int psp_sss_matmat(psp_sss_t *S, int k, const double *X_host, long ldx, double *Y_host, long ldy);
int psp_sss_matmat_dev(psp_sss_t *S, int k, const double *X_dev, long ldx, double *Y_dev, long ldy);
int psp_op_apply_block_dev(const psp_op_t *op, int k, const double *X_dev, long ldx, double *Y_dev, long ldy);

/* info[c], iter[c], relres[c] = pcg(A, B[:, c], X[:, c], tol, maxit[, K]) for c < k, the k recurrences advanced by ONE
 * loop (psp_batch.hip): q = A p is one block product, the vector updates take per-column alpha / beta, the dot products
 * of all columns finish in one reduction.  Column c ends with the info / iter / relres and the x of psp_pcg run alone on it
 * -- bit for bit: the partial sums are formed and added in the order of the loop the single solve runs (launch per phase,
 * or the one-kernel loop of small systems; beside the brick loop of 3-D grids of middle size: to rounding, as that loop
 * itself agrees with the others) -- and is frozen from then on: nothing
 * of it is written again while the loop goes on for the others.  The loop always runs in the stored numbering of A: on an
 * irregular handle whose single solves go through the renumbered copy the two differ at rounding level, like the two
 * numberings themselves.  Launches and host read-backs per iteration do not grow with k when A is native with an
 * index-free product and K is absent, a jacobi with steps = 1, or a multigrid handle (psp_last_solve_info names
 * "pcg_batch" and the launches of an iteration).  A multigrid K is applied as ONE block cycle that skips the frozen
 * columns by their device flags: an iteration is the cycle's launches_per_apply plus seven, and 16 iterations are
 * enqueued between two looks at the flags; with another product family only K is the block call.  Other products and
 * preconditioners are applied column by column inside the same loop.  A multi-device matrix gives PSP_EINVAL,
 * PSP_DEVICE=cpu PSP_ENODEV.  ldx, ldb >= n. */
int psp_pcg_batch(const psp_op_t *A, const psp_op_t *K, int n, int k, double *X_host, long ldx, const double *B_host,
                  long ldb, double tol, int maxit, int *info, int *iter, double *relres);
int psp_pcg_batch_dev(const psp_op_t *A, const psp_op_t *K, int n, int k, double *X_dev, long ldx, const double *B_dev,
                      long ldb, double tol, int maxit, int *info, int *iter, double *relres);

/* -------------------------------------------------------------------- jdsym
 * kconv, lambda, Q, it, it_inner = jdsym(A, M, K, kmax, tau, jdtol, itmax, linsolver, ...): the Jacobi-Davidson
 * eigensolver for A x = lambda M x, A and M symmetric, M positive definite or absent (jdsym.c:207-621, wrapper
 * jdsymmodule.c:128-315), every n-vector on the device.  A, M and K are ordinary operators (csr, sss, jacobi, ssor, host
 * callback); a multi-device matrix gives PSP_EINVAL, PSP_DEVICE=cpu gives PSP_ENODEV.  The correction equation
 * (correq.c:99-236) is a composite device operator, so the six Krylov loops of this library run on it unchanged
 * (linsolver = PSP_LIN_PCG .. PSP_LIN_GMRES); PSP_LIN_CALLBACK hands the two halves of it (operator, preconditioner) to
 * `linsolve` with host vectors -- the protocol of ItSolvers_Solve (jdsym.c:570-572); psp_op_apply_host applies them.
 * Deviations from the reference: the conditions jdsym.c:133-145 asserts give PSP_EINVAL; jmax is clamped to n and jmin to
 * jmax - 1; the random start vectors (jdsym.c:233-237) are uniform (0,1) from splitmix64 of (fixed seed, index), not
 * LAPACK's dlarnv, so iteration counts differ where V0 leaves columns to fill -- results are deterministic run to run.
 * lambda_host: kmax doubles in order of convergence; Q_host: n*kmax doubles, column-major; V0_host may be NULL, else
 * element (i, c) is V0_host[i*v0_row_stride + c*v0_col_stride] (strides in doubles, jdsym.c:215-228). */
#define PSP_LIN_PCG 0
#define PSP_LIN_MINRES 1
#define PSP_LIN_CGS 2
#define PSP_LIN_BICGSTAB 3
#define PSP_LIN_QMRS 4
#define PSP_LIN_GMRES 5
#define PSP_LIN_CALLBACK 6
typedef int (*psp_linsolve_fn)(void *ctx, const psp_op_t *ceA, const psp_op_t *ceK, int n, const double *b_host,
                               double *x_host, double tol, int maxit, int *info, int *iter, double *relres);
typedef struct {
  int kmax, jmax, jmin, itmax, blksize, blkwise, optype, linitmax, strategy, clvl;
  double tau, jdtol, eps_tr, toldecay;
  int linsolver;
  psp_linsolve_fn linsolve;
  void *linsolve_ctx;
  psp_host_apply_fn projector; /* x -> P x on host arrays (Jdsym_Proj, jdsym.c:239-241, :590-597), or NULL */
  void *projector_ctx;
  const double *V0_host;
  int v0_cols;
  ptrdiff_t v0_row_stride, v0_col_stride;
} psp_jdsym_params_t;
int psp_jdsym(const psp_op_t *A, const psp_op_t *M, const psp_op_t *K, int n, const psp_jdsym_params_t *p, int *kconv,
              double *lambda_host, double *Q_host, int *it_outer, int *it_inner);
/* y := op x for any operator, host vectors (the matvec / precon methods of the correction-equation object a foreign
 * linear solver is handed: correq.c:137-236) */
int psp_op_apply_host(const psp_op_t *op, const double *x_host, double *y_host);
/* Test hooks of the small dense host algebra behind jdsym (no device needed).  ritz: eigenpairs of the symmetric j x j
 * matrix whose UPPER triangle M_host holds (leading dimension ldm; the strict lower triangle is not read: jdsym.c:293-294),
 * j <= 128, by cyclic Jacobi rotations, sorted as sorteig does (jdsym.c:769-815): strategy 0 by ascending |s - tau|,
 * strategy 1 the same with every s < tau moved behind the others; ties keep ascending s.  s_host: j values, U_host: j x j
 * column-major, leading dimension ldu.  lu_factor: P H = L U in place with partial pivoting (row piv[i] was exchanged
 * with row i; PSP_ESINGULAR for an exactly zero pivot), lu_solve: w := H^-1 w (jdsym.c:536-537, correq.c:85-86). */
int psp_debug_ritz(int j, const double *M_host, int ldm, double tau, int strategy, double *s_host, double *U_host,
                   int ldu);
int psp_debug_lu_factor(int k, double *H_host, int ldh, int *piv);
int psp_debug_lu_solve(int k, const double *LU_host, int ldh, const int *piv, double *w_host);

/* ------------------------------------------ solver phase kernels (device pointers)
 * The building blocks of the loops above, exported so that the row-partitioned
 * multi-GPU driver (pysparse_amd/distributed.py) can interleave them with RCCL
 * collectives issued through torch.distributed.  Each reduction leaves its result(s) in
 * out_dev[0..k) on the device (no host synchronisation). */

/* Tell the vector kernels that v_dev[0..n) holds ONE value everywhere (checked on the device; a
 * vector that does not is simply not registered): psp_k_residual / psp_k_pupdate / psp_k_xr_update
 * then form z = dinv.*r as r_i * c without streaming dinv -- same product, 8 bytes per row less.
 * The vector must not change until psp_k_unhint.  precon.jacobi registers its own dinv. */
int psp_k_hint_constant(const double *v_dev, int n);
int psp_k_unhint(const double *v_dev);
/* out[0] = sum x_i*y_i */
int psp_k_dot(int n, const double *x_dev, const double *y_dev, double *out_dev);
/* r := b - r (pcg.c:73-74); out = { r.r, r.z } with z = dinv.*r (dinv may be NULL: z = r) */
int psp_k_residual(int n, const double *b_dev, double *r_dev, const double *dinv_dev,
                   double *out_dev);
/* p := z + beta*p (pcg.c:113-114), z = dinv.*r or r; first != 0: p := z (pcg.c:106) */
int psp_k_pupdate(int n, const double *r_dev, const double *dinv_dev, double beta, int first,
                  double *p_dev);
/* q := A p and out[0] = p.q in one pass (pcg.c:116-117); p has A.ncols entries of which
 * the first p_offset.. rows' worth are the owned ones: out = sum p[p_offset+i]*q[i] */
int psp_k_csr_matvec_dot(psp_csr_t *A, const double *p_dev, int p_offset, double *q_dev,
                         double *out_dev);
/* y := A x split around a halo exchange: rows [row_a, row_b) reference no ghost entry of x
 * and are multiplied first; wait(ctx) must return once the ghost entries have arrived (in
 * stream order); the remaining rows follow.  dot_out_dev != NULL additionally leaves
 * sum x[x_offset+i]*y[i] there (the fused p.q of pcg.c:116-117). */
typedef int (*psp_wait_fn)(void *ctx);
int psp_k_csr_matvec_overlap(psp_csr_t *A, const double *x_dev, int x_offset, double *y_dev,
                             int row_a, int row_b, psp_wait_fn wait, void *ctx, double *dot_out_dev);
/* The same update as psp_k_xr_update in the "lazy x" arrangement: the x update and
 * stagnation scan of the iteration that just finished ride in the p update of the next one.
 *   px: if xpend: scan + x += alpha_x p (p = previous direction); then p := z + beta p (first: p := z);
 *       out[0] = nonstag (meaningful when xpend)
 *   r : r -= alpha q; out = { r.r, r.z }
 *   x : the pending x update on its own (after the loop); out[0] = nonstag */
int psp_k_px_update(int n, const double *r_dev, const double *dinv_dev, double beta, int first, double alpha_x,
                    int xpend, double *p_dev, double *x_dev, double *out_dev);
int psp_k_r_update(int n, double alpha, const double *q_dev, const double *dinv_dev, double *r_dev,
                   double *out_dev);
int psp_k_x_update(int n, double alpha, const double *p_dev, double *x_dev, double *out_dev);
/* stagnation scan + x += alpha p, r -= alpha q (pcg.c:127-143) and
 * out = { r.r, r.z (z = dinv.*r), nonstag } where nonstag != 0 iff 1 + dmax != 1 */
int psp_k_xr_update(int n, double alpha, const double *p_dev, const double *q_dev,
                    const double *dinv_dev, double *x_dev, double *r_dev, double *out_dev);
/* y := x .* dinv (jacobi(), preconmodule.c:41-42) on device vectors */
int psp_k_jacobi(int n, const double *x_dev, const double *dinv_dev, double *y_dev);
/* gather send_dev[i] = v[idx[i]] (halo packing) */
int psp_k_gather(int count, const int *idx_dev, const double *v_dev, double *send_dev);

/* Test hook (tests/test_gpu_vec_passes.py): ONE launch of a fused vector pass of the cgs / bicgstab / qmrs / gmres / minres
 * loops or of the Jacobi preconditioner, which otherwise run only inside whole solves.  vec_dev[0 .. nvec) are the pass's
 * device vectors in the order below, scal_host[0 .. nscal) its by-value scalars; dinv_dev is the Jacobi array of the
 * passes marked [K] (NULL: no preconditioner; a vector registered with psp_k_hint_constant: the constant form) and of
 * JACOBI_SWEEP, NULL for every other pass.  Vectors in (parentheses) are dereferenced only with dinv_dev and may be NULL
 * without it.  sums_dev receives the finished reductions {in braces}; it is ignored for passes that reduce nothing.
 *   LIN2            x y z                 a b                    z = a x + b y (z may be x or y)
 *   SCAL            x                     a                      x = a x
 *   BICG_P     [K]  r v p (phat)          beta omega             p = r + beta (p - omega v), FIRST: p = r; phat = K p
 *   BICG_S     [K]  r v s (shat)          alpha                  s = r - alpha v; shat = K s
 *   BICG_XR         x phat shat s t r rhat  alpha omega          x += alpha phat + omega shat; r = s - omega t  {r.r, rhat.r}
 *   CGS_Q      [K]  u v x q tmp2          alpha                  q = u - alpha v; tmp2 = K (u + q); x += alpha tmp2
 *   CGS_R           r t r0                alpha                  r -= alpha t  {r.r, r.r0}
 *   CGS_P      [K]  r q p u (kp)          beta                   u = r + beta q; p = u + beta (q + beta p); kp = K p
 *   QMRS_KV    [K]  v1 (wrk1)             -                      wrk1 = K v1  {wrk1.v1; without K: v1.v1}
 *   QMRS_PG         v1 wrk1 p g           cc                     p = v1 - cc p; g = wrk1 - cc g
 *   QMRS_V          t v1                  beta                   v1 = t - beta v1  {v1.v1}
 *   QMRS_DX    [K]  p d x v1 (wrk1)       eta cc rho1inv         d = eta p + cc d; x += d; v1 *= rho1inv; wrk1 = K v1  {wrk1.v1}
 *   AXPY_DOT        x y z                 a                      y += a x  {y.z; z NULL: y.y}.  COEF_DEV: a = -scal[0], read
 *                                                                from the device
 *   AXPY_DOT_CHAIN  prev h_out x y z      np_prev                h = sum of prev[0 .. np_prev), np_prev in 1 .. 4096; *h_out = h;
 *                                                                y -= h x  {y.z; z NULL: y.y}.  PREV_WS: prev is NULL and
 *                                                                stands for the partial sums the calling thread's last
 *                                                                reducing call of this function left (np_prev must be their count)
 *   JACOBI_SWEEP    x temp y              -                      y = (x - y) dinv + temp
 *   DINV            diag dinv             omega                  dinv = omega / diag  {number of entries with 1 + d == 1}
 *   SCALE_DIV       y v                   beta                   v = y / beta
 *   LANCZOS    [K]  av v_hat v_hat_old (y)  c1 c2                v_hat_old = av - c1 v_hat - c2 v_hat_old; y = K v_hat_old
 *                                                                {v_hat_old.y; without K: v_hat_old.v_hat_old}
 *   LANCZOS_PLAIN   av v_hat v_hat_old    c1 c2                  the same without K and without the sum
 *   MINRES_WX       v w w_old x           r1 r2 r3 c_eta vdiv    w_old = (v - r3 w_old - r2 w) / r1; x += c_eta w_old;
 *                                                                SCALED: v / vdiv in place of v
 *   MINRES_WX_VNEXT v ynext w w_old x     -                      the same with the scalars of a NULL device state
 *                                                                (r1 = r2 = r3 = c_eta = 0) and v = ynext / 1
 * (the two MINRES passes run without a device state; their device-state forms are psp_kd_minres_*.)
 * PSP_VEC_DEVSCAL (the nine passes that take their scalars from a device state: BICG_*, CGS_*, QMRS_PG / _V / _DX): the
 * scalars travel in registers i0, i1, i2 (distinct, 0 .. 31) of a KryDev whose other registers hold NaN and whose iteration
 * counter is `iter` (BICG_P takes "first" from iter == 1, not from PSP_VEC_FIRST); the by-value arguments of the launch are
 * NaN.  PSP_VEC_STATUS_SET (with DEVSCAL): the state says the loop has ended -- the pass must change nothing.
 * PSP_EINVAL before anything is launched: an unknown pass, other counts than the table's, n < 1, a flag the pass does not
 * take, a NULL vector the selected form dereferences, dinv_dev where the pass takes none.
 * psp_debug_vec_form: the form the calling thread's last vector-kernel launch took -- *V = 2 (one 16-byte access per lane)
 * or 1 (two 8-byte ones), *pre = 0 (no preconditioner), 1 (dinv array) or 2 (constant); both 0 before the first launch. */
enum {
  PSP_VEC_LIN2 = 0, PSP_VEC_SCAL, PSP_VEC_BICG_P, PSP_VEC_BICG_S, PSP_VEC_BICG_XR, PSP_VEC_CGS_Q, PSP_VEC_CGS_R,
  PSP_VEC_CGS_P, PSP_VEC_QMRS_KV, PSP_VEC_QMRS_PG, PSP_VEC_QMRS_V, PSP_VEC_QMRS_DX, PSP_VEC_AXPY_DOT,
  PSP_VEC_AXPY_DOT_CHAIN, PSP_VEC_JACOBI_SWEEP, PSP_VEC_DINV, PSP_VEC_SCALE_DIV, PSP_VEC_LANCZOS, PSP_VEC_LANCZOS_PLAIN,
  PSP_VEC_MINRES_WX, PSP_VEC_MINRES_WX_VNEXT, PSP_VEC_NPASS
};
#define PSP_VEC_FIRST 1u
#define PSP_VEC_SCALED 2u
#define PSP_VEC_DEVSCAL 4u
#define PSP_VEC_STATUS_SET 8u
#define PSP_VEC_COEF_DEV 16u
#define PSP_VEC_PREV_WS 32u
int psp_debug_vec_pass(int pass, int n, double *const *vec_dev, int nvec, const double *dinv_dev, const double *scal_host,
                       int nscal, unsigned flags, int i0, int i1, int i2, int iter, double *sums_dev);
int psp_debug_vec_form(int *V, int *pre);

/* ------------------------------------------ device-resident solver state for the multi-GPU driver
 * The same loops with NO host round trip per reduction: alpha / beta / the exit tests of pcg.c:100-162
 * (resp. the Lanczos / Givens recurrences of minres.c:129-192) live in a small device-side state; the
 * psp_kd_* kernels read their coefficients from it and turn into no-ops once the loop has ended.  One
 * iteration is cut at its two reductions so that an all-reduce can be issued in stream order between
 * "finish the local partial sums" (out_dev) and "take the reference's branches on the reduced values"
 * (psp_kd_*_scalar*).  The host enqueues a batch of iterations, then calls *_fetch once. */
typedef struct psp_pcgstate psp_pcgstate_t;
typedef struct {
  int status;      /* 0 running, 1 finished */
  int info, iter;  /* valid when finished (pend_maxit: decided by the final x update, see below) */
  int it;          /* iteration the enqueued kernels are working on */
  int xpend;       /* x += alpha_x p of the last finished iteration is still to be applied (psp_k_x_update) */
  int stag0;       /* alpha == 0 in that iteration (pcg.c:124-125) */
  int pend_maxit;  /* the loop ran out: -5 or -1 is decided by the stagnation scan of the final x update */
  double relres, normr, n2b, alpha_x;
} psp_pcg_status_t;
int psp_pcgstate_create(psp_pcgstate_t **out);
int psp_pcgstate_destroy(psp_pcgstate_t *st);
/* state at the head of iteration 1: ||b||, tol*||b||, ||r0||, rho0 = r0.z0 (all already reduced over ranks) */
int psp_pcgstate_init(psp_pcgstate_t *st, double n2b, double tolb, double normr0, double rho0, int maxit,
                      int want_hist);
int psp_pcgstate_fetch(psp_pcgstate_t *st, psp_pcg_status_t *out); /* synchronises the stream */
int psp_pcgstate_hist(psp_pcgstate_t *st, int first, int count, double *hist_host);
/* lazy-x arrangement, scalars from the state:
 *   px: pending x update + scan, then p := z + beta p;  out[0] = local nonstag count
 *   matvec_overlap: q := A p around the halo wait;       dot_out[0] = local p.q
 *   scalar_xpq(scal = {p.q, nonstag} after the all-reduce): pcg.c:159-162 of the previous iteration,
 *       :101-112 of this one, alpha (:117-125)
 *   r : r -= alpha q;                                    out = local {r.r, r.z}
 *   scalar_r(scal = {r.r, r.z} after the all-reduce): pcg.c:152-157, next rho / beta */
int psp_kd_px_update(const psp_pcgstate_t *st, int n, const double *r_dev, const double *dinv_dev, double *p_dev,
                     double *x_dev, double *out_dev);
int psp_kd_csr_matvec_overlap(const psp_pcgstate_t *st, psp_csr_t *A, const double *x_dev, int x_offset,
                              double *y_dev, int row_a, int row_b, psp_wait_fn wait, void *ctx,
                              double *dot_out_dev);
int psp_kd_pcg_scalar_xpq(psp_pcgstate_t *st, const double *scal_dev);
int psp_kd_r_update(const psp_pcgstate_t *st, int n, const double *q_dev, const double *dinv_dev, double *r_dev,
                    double *out_dev);
int psp_kd_pcg_scalar_r(psp_pcgstate_t *st, const double *scal_dev);

typedef struct psp_minresstate psp_minresstate_t;
typedef struct {
  int status;  /* ended by -3 / -6 (minres.c:144-146, :160-162), or after the last w/x update */
  int stop;    /* the loop test of minres.c:114 failed: finished once the enqueued w/x update has run */
  int info, iter;
  double relres;   /* written on the 0 / -1 exits only, as in the reference */
  double norm_rmr;
} psp_minres_status_t;
int psp_minresstate_create(psp_minresstate_t **out);
int psp_minresstate_destroy(psp_minresstate_t *st);
/* state at the head of iteration 1: ||r0||, beta = sqrt(v_hat . y) (reduced over ranks), tol, maxit */
int psp_minresstate_init(psp_minresstate_t *st, double norm_r0, double beta0, double errtol, int it_max,
                         int want_hist);
int psp_minresstate_fetch(psp_minresstate_t *st, psp_minres_status_t *out);
int psp_minresstate_hist(psp_minresstate_t *st, int first, int count, double *hist_host);
/* one iteration of minres.c:96-193 on a row block:
 *   scale:   v := y / beta (:123-124)        matvec: Av := A v around the halo wait, dot_out = local v.Av
 *   scalar(0, {v.Av} reduced): alpha, the Lanczos coefficients (:129-131)
 *   lanczos: v_hat_old := Av - c1 v_hat - c2 v_hat_old (the caller swaps the names), y := dinv .* it,
 *            out = local v_hat.y
 *   scalar(1, {v_hat.y} reduced): beta, Givens rotation, the exits, the loop test of the next iteration
 *   wx:      w_old := (v - r3 w_old - r2 w) / r1 (the caller swaps the names); x += c eta w (:172-180) */
int psp_kd_minres_scale(const psp_minresstate_t *st, int n, const double *y_dev, double *v_dev);
int psp_kd_minres_matvec(const psp_minresstate_t *st, psp_csr_t *A, const double *v_dev, int v_offset,
                         double *av_dev, int row_a, int row_b, psp_wait_fn wait, void *ctx, double *dot_out_dev);
int psp_kd_minres_lanczos(const psp_minresstate_t *st, int n, const double *av_dev, const double *v_hat_dev,
                          double *v_hat_old_dev, const double *dinv_dev, double *y_dev, double *out_dev);
int psp_kd_minres_scalar(psp_minresstate_t *st, int which, const double *scal_dev);
int psp_kd_minres_wx(const psp_minresstate_t *st, int n, const double *v_dev, const double *w_dev,
                     double *w_old_dev, double *x_dev);

#ifdef __cplusplus
}
#endif
#endif /* PYSPARSE_HIP_H */
