// psp_batch.hip -- PCG for k right-hand sides in lockstep: pcg.c:57-166 run by ONE loop that advances k recurrences.
//
// Per iteration (A native with an index-free product, K absent or jacobi with steps = 1 -- five launches whatever k is):
//     pupdate   P[:, c] = z + beta_c P[:, c]                    (z = R[:, c] .* dinv or R[:, c]; first iteration: P = z)
//     product   Q = A P, one block product (psp_spmm.hip) that also leaves the p.q partial sums of every column
//     finish    one workgroup per column adds its partial sums, then takes pcg.c:117-125 for that column
//     xr        stagnation scan, X += alpha_c P, R -= alpha_c Q, partial sums of r.r, r.z and the scan
//     finish    one workgroup per column: pcg.c:127-162 and the head of the next iteration (pcg.c:99-112)
// Other operators keep the same loop and the same arithmetic; what cannot be batched is done column by column in its place:
// a native product with another kernel family runs the single-vector product (its fused dot has that kernel's own order
// of partial sums), any other preconditioner is applied column by column and followed by a batched r.z dot.
// K = precon.multigrid: z = K r is ONE block cycle (psp_mg.hip) that skips the frozen columns by
// the device flags; with the block product beside it the loop enqueues 16 iterations between two looks at the flags,
// as the fused path does, and an iteration is the cycle's launches plus seven (r.z, head, pupdate, product, finish, xr,
// finish) whatever k is.  With another product family only K becomes the block call; the rest stays column by column
// with a look at the flags after every iteration.
//
// Bit equality with psp_pcg, column by column: the element a thread owns (2t, 2t+1 of a 512-row span), the order in which
// it adds, the wave tree, the four waves left to right and reduce_block over the spans are those of dot_kernel,
// residual_kernel, x_update_kernel, r_update_kernel (psp_vec.hip) and of csr_spmv_w4's fused dot; the scalar steps are
// pcg_head / pcg_alpha / pcg_tail of psp_recur.h -- the ones every loop of psp_pcg takes -- applied to one column's
// state.  One exception is followed on purpose:
// a small system that psp_pcg hands to the one-kernel loop of psp_coop.hip is reduced in that loop's own order (a row per
// thread, wave sums, the 16 waves of a workgroup of 1024 rows, then the workgroups, each left to right), because that is
// what the single solve of such a system computes; p.q is then a batched dot of its own behind the block product (six
// launches per iteration).  The brick loop of psp_mid.hip (3-D grids of middle size) deals its points out in bricks and
// agrees with every other loop to rounding only; so does a column of this loop beside it.
// Which loop the single solve is, by size (tests/test_gpu_block_sizes.py asserts each name): pcg_coop or, from 2^15 rows of
// an offset-structured system, pcg_mid / pcg_brick; where none of them applies -- varying coefficients beyond 2^20 rows,
// another kernel family, a handle without CSR arrays (psp_csr_poisson_big, psp_csr_release_arrays) at any size, or
// psp_set_single_kernel_loops(0) -- the lazy launch-per-phase loop pcg_lazy, and pcg_lazy_pf (p and x updates folded into
// the product) from 2^21 rows.  Those two put off the x update by one phase and, beyond 4096 partial sums, fold them in two
// launches; the operands and the order of every sum are the eager loop's, so this loop's columns carry their bits as well.
//
// Freezing: a column whose exit is decided (info 0, -2, -5, -6, or -1 with iter = maxit + 1) sets its flag on the device;
// every kernel skips flagged columns, so nothing of a frozen column is written again.  The loop ends when all are frozen.
// The loop always runs in the stored numbering of A (csr_spmv_launch_stored; the block kernels know no other).
#include <algorithm>
#include <vector>

#include "psp_internal.h"

namespace psp {
namespace {

typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

constexpr int kBlock = 256;
constexpr int kMaxN = 1 << 25;  // 65 536 spans: what ONE finishing workgroup adds in the canonical order (psp_internal.h)

// one column's recurrence on the device: PcgCol of psp_recur.h
using BatchCol = PcgCol;

// per thread: partial sums (3 values x k columns x spans), the columns' states and their frozen flags, with a pinned
// mirror of both; for the stream the thread used last (as psp_bvec.hip's set).  psp_trim releases it (batch_trim).
struct BatchScratch {
  int device = -1;
  hipStream_t last = nullptr;
  double *parts = nullptr;
  size_t parts_cap = 0;
  BatchCol *st = nullptr, *st_host = nullptr;
  int *frozen = nullptr, *frozen_host = nullptr;
  double *red = nullptr, *red_host = nullptr;  // 2 sums per column (set-up of a solve)
  int cols_cap = 0;
};
thread_local BatchScratch tl_batch;

void batch_release(BatchScratch &s) {
  if (s.parts || s.st || s.frozen) {
    int cur = -1;
    const bool moved = s.device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != s.device;
    if (moved) (void)hipSetDevice(s.device);
    (void)hipDeviceSynchronize();
    if (s.parts) (void)hipFree(s.parts);
    if (s.st) (void)hipFree(s.st);
    if (s.frozen) (void)hipFree(s.frozen);
    if (s.st_host) (void)hipHostFree(s.st_host);
    if (s.frozen_host) (void)hipHostFree(s.frozen_host);
    if (s.red) (void)hipFree(s.red);
    if (s.red_host) (void)hipHostFree(s.red_host);
    if (moved) (void)hipSetDevice(cur);
    (void)hipGetLastError();
  }
  s = BatchScratch();
}

int batch_scratch(size_t parts_needed, int cols, BatchScratch **out) {
  BatchScratch &s = tl_batch;
  const int d = current_device();
  if (s.device != d || s.last != stream()) {
    batch_release(s);
    s.device = d;
    s.last = stream();
  }
  if (parts_needed > s.parts_cap) {
    if (s.parts) {
      PSP_HIP(hipStreamSynchronize(stream()));
      (void)hipFree(s.parts);
      s.parts = nullptr;
      s.parts_cap = 0;
    }
    PSP_HIP(hipMalloc((void **)&s.parts, sizeof(double) * parts_needed));
    s.parts_cap = parts_needed;
  }
  if (cols > s.cols_cap) {
    PSP_HIP(hipStreamSynchronize(stream()));
    if (s.st) (void)hipFree(s.st);
    if (s.frozen) (void)hipFree(s.frozen);
    if (s.st_host) (void)hipHostFree(s.st_host);
    if (s.frozen_host) (void)hipHostFree(s.frozen_host);
    if (s.red) (void)hipFree(s.red);
    if (s.red_host) (void)hipHostFree(s.red_host);
    s.st = s.st_host = nullptr;
    s.frozen = s.frozen_host = nullptr;
    s.red = s.red_host = nullptr;
    s.cols_cap = 0;
    const int cap = std::max(cols, 16);
    PSP_HIP(hipMalloc((void **)&s.st, sizeof(BatchCol) * cap));
    PSP_HIP(hipMalloc((void **)&s.frozen, sizeof(int) * cap));
    PSP_HIP(hipHostMalloc((void **)&s.st_host, sizeof(BatchCol) * cap));
    PSP_HIP(hipHostMalloc((void **)&s.frozen_host, sizeof(int) * cap));
    PSP_HIP(hipMalloc((void **)&s.red, sizeof(double) * 2 * cap));
    PSP_HIP(hipHostMalloc((void **)&s.red_host, sizeof(double) * 2 * cap));
    s.cols_cap = cap;
  }
  *out = &s;
  return PSP_OK;
}

// ---------------------------------------------------------------- vector kernels: grid (spans, columns)
// Thread t owns elements 2t and 2t+1 of its span, as in psp_vec.hip: the pair is one 8-byte-aligned 16-byte access when
// both exist.  partials[(v*k + c)*pstride + span] is value v of column c.

__device__ __forceinline__ void block_store(double v, double *__restrict__ dst, double (*sh)[4], int j) {
  const double s = psp_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *dst = sh[j][0] + sh[j][1] + sh[j][2] + sh[j][3];
}

// x . y per column (dot_kernel)
__global__ __launch_bounds__(kBlock) void bdot_kernel(long n, int k, const double *__restrict__ X, long ldx,
                                                      const double *__restrict__ Y, long ldy,
                                                      double *__restrict__ partials, long pstride,
                                                      const int *__restrict__ frozen, int coop) {
  __shared__ double sh[1][4];
  const int c = blockIdx.y;
  if (frozen && frozen[c]) return;
  const double *x = X + (size_t)c * ldx, *y = Y + (size_t)c * ldy;
  if (coop) {  // one row per thread, one partial sum per wave of 64 rows (psp_coop.hip)
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    const double s = psp_wave_sum(i < n ? x[i] * y[i] : 0.0);
    if ((threadIdx.x & 63) == 0) partials[(size_t)c * pstride + blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)] = s;
    return;
  }
  const long i = (long)blockIdx.x * kVecSpan + 2 * threadIdx.x;
  double acc = 0.0;
  if (i + 1 < n) {
    const d2u a = *reinterpret_cast<const d2u *>(x + i), b = *reinterpret_cast<const d2u *>(y + i);
    acc += a.x * b.x;
    acc += a.y * b.y;
  } else if (i < n) {
    acc += x[i] * y[i];
  }
  block_store(acc, partials + (size_t)c * pstride + blockIdx.x, sh, 0);
}

// r = b - r; partials {r.r, r.z}, z = dinv .* r or r (residual_kernel)
__global__ __launch_bounds__(kBlock) void bresidual_kernel(long n, int k, const double *__restrict__ B, long ldb,
                                                           double *__restrict__ R, long ldr,
                                                           const double *__restrict__ dinv,
                                                           double *__restrict__ partials, long pstride) {
  __shared__ double sh[2][4];
  const int c = blockIdx.y;
  const double *b = B + (size_t)c * ldb;
  double *r = R + (size_t)c * ldr;
  const long i = (long)blockIdx.x * kVecSpan + 2 * threadIdx.x;
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (i + u < n) {
      const double t = b[i + u] - r[i + u];
      r[i + u] = t;
      acc0 += t * t;
      if (dinv) {
        const double z = t * dinv[i + u];
        acc1 += t * z;
      }
    }
  }
  if (!dinv) acc1 = acc0;
  block_store(acc0, partials + (size_t)c * pstride + blockIdx.x, sh, 0);
  block_store(acc1, partials + (size_t)(k + c) * pstride + blockIdx.x, sh, 1);
}

// p = z + beta p, or p = z in a column's first iteration; z = Z .* dinv or Z (pupdate_kernel)
__global__ __launch_bounds__(kBlock) void bpupdate_kernel(long n, const double *__restrict__ Z, long ldz,
                                                          const double *__restrict__ dinv, double *__restrict__ P,
                                                          long ldp, const BatchCol *__restrict__ st,
                                                          const int *__restrict__ frozen) {
  const int c = blockIdx.y;
  if (frozen[c]) return;
  const double beta = st[c].beta;
  const bool first = st[c].it == 1;
  const double *zc = Z + (size_t)c * ldz;
  double *p = P + (size_t)c * ldp;
  const long i = (long)blockIdx.x * kVecSpan + 2 * threadIdx.x;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (i + u < n) {
      double z = zc[i + u];
      if (dinv) z = z * dinv[i + u];
      if (!first) z = z + beta * p[i + u];
      p[i + u] = z;
    }
  }
}

// pcg.c:127-152: stagnation scan + x += alpha p (x_update_kernel), r -= alpha q and {r.r, r.z} (r_update_kernel)
__global__ __launch_bounds__(kBlock) void bxr_kernel(long n, int k, const double *__restrict__ P, long ldp,
                                                     const double *__restrict__ Q, long ldq,
                                                     const double *__restrict__ dinv, double *__restrict__ X, long ldx,
                                                     double *__restrict__ R, long ldr, const BatchCol *__restrict__ st,
                                                     const int *__restrict__ frozen, double *__restrict__ partials,
                                                     long pstride, int coop) {
  __shared__ double sh[3][4];
  const int c = blockIdx.y;
  if (frozen[c]) return;
  const double alpha = st[c].alpha;
  const bool upd = alpha != 0.0;
  const double malpha = -alpha;
  const double *p = P + (size_t)c * ldp, *q = Q + (size_t)c * ldq;
  double *x = X + (size_t)c * ldx, *r = R + (size_t)c * ldr;
  if (coop) {  // the same element arithmetic, one row per thread and one partial sum per wave of 64 rows (psp_coop.hip)
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    if (i < n) {
      const double pp = p[i], xx = x[i];
      const double ddum = (xx != 0.0) ? fabs(alpha * pp / xx) : ((pp != 0.0) ? 1.0 : 0.0);
      const double dm = (ddum > 0.0) ? ddum : 0.0;
      if (upd) x[i] = xx + alpha * pp;
      const double rr = r[i];
      const double t = upd ? rr + malpha * q[i] : rr;
      r[i] = t;
      v0 = t * t;
      v1 = t * (dinv ? t * dinv[i] : t);
      v2 = (1.0 + dm != 1.0) ? 1.0 : 0.0;
    }
    const double s0 = psp_wave_sum(v0), s1 = psp_wave_sum(v1), s2 = psp_wave_sum(v2);
    if ((threadIdx.x & 63) == 0) {
      const size_t w = (size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
      partials[(size_t)c * pstride + w] = s0;
      partials[(size_t)(k + c) * pstride + w] = s1;
      partials[(size_t)(2 * k + c) * pstride + w] = s2;
    }
    return;
  }
  const long i = (long)blockIdx.x * kVecSpan + 2 * threadIdx.x;
  double dmax = 0.0, acc0 = 0.0, acc1 = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (i + u < n) {
      const double pp = p[i + u], xx = x[i + u];
      const double quot = fabs(alpha * pp / xx);
      const double ddum = (xx != 0.0) ? quot : ((pp != 0.0) ? 1.0 : 0.0);
      dmax = (ddum > dmax) ? ddum : dmax;
      if (upd) x[i + u] = xx + alpha * pp;
      const double rr = r[i + u];
      const double t = upd ? rr + malpha * q[i + u] : rr;
      r[i + u] = t;
      acc0 += t * t;
      if (dinv) {
        const double z = t * dinv[i + u];
        acc1 += t * z;
      }
    }
  }
  if (!dinv) acc1 = acc0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(dmax, off, 64);
    if (o > dmax) dmax = o;
  }
  const double ns = ((threadIdx.x & 63) == 0 && (1.0 + dmax != 1.0)) ? 1.0 : 0.0;
  block_store(acc0, partials + (size_t)c * pstride + blockIdx.x, sh, 0);
  block_store(acc1, partials + (size_t)(k + c) * pstride + blockIdx.x, sh, 1);
  block_store(ns, partials + (size_t)(2 * k + c) * pstride + blockIdx.x, sh, 2);
}

// ---------------------------------------------------------------- scalar steps, one column each

enum { kStepHead = 0, kStepPq = 1, kStepXr = 2 };

// one workgroup per column: the column's values in reduce_block's order, then the step that waits for them.
// kStepXr, fused != 0: r.z of the update is the next iteration's rho (z = dinv .* r or r): the head follows at once
template <int STEP>
__global__ __launch_bounds__(kReduceBlock) void bfinish_kernel(const double *__restrict__ parts, int nparts,
                                                               long pstride, int k, BatchCol *st, int *frozen,
                                                               int fused, int coop_nwg) {
  __shared__ double sh[kOneBlockGroups];
  __shared__ double out[3];
  const int c = blockIdx.x;
  if (frozen[c]) return;
  constexpr int NV = STEP == kStepXr ? 3 : 1;
  if (coop_nwg > 0) {
    // the order of psp_coop.hip (block_sum, grid_sum): the 16 wave sums of a workgroup of 1024 rows left to right from
    // 0.0, then the workgroups left to right from 0.0 (one workgroup: its sum as it is); nparts wave sums are stored
    for (int j = 0; j < NV; ++j) {
      const double *p = parts + (size_t)c * pstride + (size_t)j * k * pstride;
      if ((int)threadIdx.x < coop_nwg) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) {
          const int idx = threadIdx.x * 16 + w;
          t += idx < nparts ? p[idx] : 0.0;
        }
        sh[threadIdx.x] = t;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        double tot = sh[0];
        if (coop_nwg > 1) {
          tot = 0.0;
          for (int g = 0; g < coop_nwg; ++g) tot += sh[g];
        }
        out[j] = tot;
      }
      __syncthreads();
    }
  } else {
    reduce_block(parts + (size_t)c * pstride, nparts, NV, (int)((long)k * pstride), true, out, sh);
  }
  if (threadIdx.x != 0) return;
  // the column's step (psp_recur.h); an exit freezes the column
  BatchCol &s = st[c];
  bool over;
  if constexpr (STEP == kStepHead) {
    over = pcg_head(s, out[0]);
  } else if constexpr (STEP == kStepPq) {
    over = pcg_alpha(s, out[0]);
  } else {
    over = pcg_tail(s, sqrt(out[0]), out[2] == 0.0) || (fused && pcg_head(s, out[1]));
  }
  if (over) frozen[c] = 1;
}

// out[v*k + c] = value v of column c, nothing else (the set-up's norms)
__global__ __launch_bounds__(kReduceBlock) void breduce_kernel(const double *__restrict__ parts, int nparts, long pstride,
                                                               int k, int nvals, double *__restrict__ out) {
  __shared__ double sh[kOneBlockGroups];
  __shared__ double val[2];
  const int c = blockIdx.x;
  reduce_block(parts + (size_t)c * pstride, nparts, nvals, (int)((long)k * pstride), true, val, sh);
  if (threadIdx.x == 0)
    for (int v = 0; v < nvals; ++v) out[(size_t)v * k + c] = val[v];
}

// the sums to the host (synchronises)
int reduce_fetch_cols(BatchScratch *bs, int nparts, long pstride, int k, int nvals) {
  hipLaunchKernelGGL(breduce_kernel, dim3(k), dim3(nparts > kTailGroup ? kReduceBlock : 64), 0, stream(), bs->parts, nparts,
                     pstride, k, nvals, bs->red);
  PSP_LAUNCH_CHECK();
  PSP_HIP(hipMemcpyAsync(bs->red_host, bs->red, sizeof(double) * (size_t)nvals * k, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

template <int STEP>
int finish_step(const double *parts, int nparts, long pstride, int k, int col0, int cols, BatchCol *st, int *frozen,
                int fused, int coop_nwg = 0) {
  if ((long)k * pstride > 0x7fffffffL) return fail(PSP_EINVAL, "psp_pcg_batch: k * n too large for the partial-sum buffer");
  hipLaunchKernelGGL((bfinish_kernel<STEP>), dim3(cols),
                     dim3(coop_nwg > 0 ? 256 : (nparts > kTailGroup ? kReduceBlock : 64)), 0, stream(),
                     parts + (size_t)col0 * pstride, nparts, pstride, k, st + col0, frozen + col0, fused, coop_nwg);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

const double *fused_dinv(const psp_op *K) {
  if (K && K->kind == PSP_OP_JACOBI && K->jac->steps == 1) return K->jac->dinv;
  return nullptr;
}

struct BlockVecs {
  std::vector<std::pair<double *, size_t>> held;
  ~BlockVecs() {
    for (auto &h : held) scratch_put(h.first, h.second);
  }
  int alloc(size_t n, double **out) {
    PSP_TRY(scratch_get(n, out));
    held.push_back({*out, n});
    return PSP_OK;
  }
};

}  // namespace

void batch_trim() { batch_release(tl_batch); }

// the loop at its device-pointer level: handles locked, arguments checked
int pcg_batch_dev(const psp_op *A, const psp_op *K, int n, int k, double *X, long ldx, const double *B, long ldb,
                  double tol, int maxit, int *info, int *iter, double *relres) {
  note_solve("pcg_batch", 0, -1, 0);
  Workspace *w;
  PSP_TRY(workspace(&w));
  const psp_csr *Acsr = op_native_csr(A);
  if (Acsr) PSP_TRY(csr_spmm_check("psp_pcg_batch", Acsr));
  const double *dinv = fused_dinv(K);
  // "fused" as in pcg_device_core: z = dinv .* r (or r) is formed on the fly and r.z comes with the r update
  const bool fused = Acsr != nullptr && (K == nullptr || dinv != nullptr);
  const double *fd = fused ? dinv : nullptr;
  const int spans = vec_grid(*w, n);
  W4View view;
  int w4 = 0;
  if (Acsr) PSP_TRY(csr_w4_view(Acsr, &view, &w4));
  // Which order the single solve adds in: systems that psp_pcg hands to the one-kernel loop of psp_coop.hip (small, rows of
  // at most 8 entries, neither of the psp_mid.hip loops taking them first) are reduced in THAT loop's order -- a row per
  // thread, wave sums, workgroups of 1024 rows -- which differs from the launch-per-phase order at rounding level.
  // The question is put for rho != 0: the residuals are not formed yet.  A single solve whose first rho IS 0 skips the
  // psp_mid.hip loops (PcgSkLoop::needs_rho) and may go to psp_coop.hip where this says it would not; that solve ends in
  // its first iteration (pcg.c:101-104) before anything is added, so the two answers are kept as they are.
  const bool coop_order = fused && maxit >= 1 && single_kernel_loops_enabled() && pcg_sk_choice(Acsr, n, true) == pcg_coop_loop;
  const int cgrid = (n + kBlock - 1) / kBlock, cwaves = cgrid * (kBlock / 64), cnwg = (n + 1023) / 1024;
  const long pstride = std::max(std::max(spans, w4 ? view.grid : 0), coop_order ? cwaves : 0);
  BatchScratch *bs;
  PSP_TRY(batch_scratch((size_t)3 * k * pstride, k, &bs));
  double *parts = bs->parts;
  BatchCol *st = bs->st, *sh = bs->st_host;
  int *frozen = bs->frozen, *fh = bs->frozen_host;
  BlockVecs mem;
  double *R, *P, *Q, *Z = nullptr;
  const size_t nk = (size_t)n * k;
  PSP_TRY(mem.alloc(nk, &R));
  PSP_TRY(mem.alloc(nk, &P));
  PSP_TRY(mem.alloc(nk, &Q));
  if (!fused && K) PSP_TRY(mem.alloc(nk, &Z));
  std::vector<double> s((size_t)2 * k);
  const dim3 vgrid(spans, k);

  // n2b = ||b|| (pcg.c:57)
  hipLaunchKernelGGL(bdot_kernel, vgrid, dim3(kBlock), 0, stream(), (long)n, k, B, ldb, B, ldb, parts, pstride,
                     (const int *)nullptr, 0);
  PSP_LAUNCH_CHECK();
  if ((long)k * pstride > 0x7fffffffL) return fail(PSP_EINVAL, "psp_pcg_batch: k * n too large for the partial-sum buffer");
  PSP_TRY(reduce_fetch_cols(bs, spans, pstride, k, 1));
  std::vector<double> n2b(k), tolb(k), normr(k), rho0(k);
  std::vector<char> decided(k, 0);
  for (int c = 0; c < k; ++c) {
    PSP_TRY(robust_norm2(n, B + (size_t)c * ldb, bs->red_host[c], &n2b[c]));
    tolb[c] = tol * n2b[c];
    info[c] = -1;  // pcg.c:70
    iter[c] = 0;
    relres[c] = 0.0;
  }
  // r = b - A x, normr (pcg.c:72-75); x0 of every column is read, none is written
  if (Acsr)
    PSP_TRY(csr_spmm_launch(Acsr, k, X, ldx, R, n, nullptr, nullptr, 0, nullptr));
  else
    for (int c = 0; c < k; ++c) PSP_TRY(op_apply(A, X + (size_t)c * ldx, R + (size_t)c * n));
  hipLaunchKernelGGL(bresidual_kernel, vgrid, dim3(kBlock), 0, stream(), (long)n, k, B, ldb, R, (long)n, fd, parts,
                     pstride);
  PSP_LAUNCH_CHECK();
  PSP_TRY(reduce_fetch_cols(bs, spans, pstride, k, 2));
  for (int c = 0; c < k; ++c) {
    s[c] = bs->red_host[c];
    rho0[c] = bs->red_host[k + c];
  }
  int running = 0;
  for (int c = 0; c < k; ++c) {
    fh[c] = 1;
    decided[c] = 1;
    if (n2b[c] == 0.0) {  // pcg.c:58-67
      PSP_HIP(hipMemsetAsync(X + (size_t)c * ldx, 0, sizeof(double) * (size_t)n, stream()));
      info[c] = 0;
      continue;
    }
    PSP_TRY(robust_norm2(n, R + (size_t)c * n, s[c], &normr[c]));
    if (normr[c] <= tolb[c]) {  // pcg.c:77-84
      info[c] = 0;
      relres[c] = normr[c] / n2b[c];
      continue;
    }
    if (maxit < 1) {  // the loop does not run: pcg.c:165-166
      iter[c] = 1;
      relres[c] = normr[c] / n2b[c];
      continue;
    }
    if (fused && rho0[c] == 0.0) {  // pcg.c:101-104 in iteration 1
      info[c] = -2;
      iter[c] = 1;
      relres[c] = normr[c] / n2b[c];
      continue;
    }
    fh[c] = 0;
    decided[c] = 0;
    ++running;
  }
  for (int c = 0; c < k; ++c) {
    BatchCol b = BatchCol();
    b.rho = fused ? rho0[c] : 1.0;
    b.rho1 = 1.0;
    b.normr = normr[c];
    b.tolb = tolb[c];
    b.n2b = n2b[c];
    b.it = 1;
    b.maxit = maxit;
    sh[c] = b;
  }
  PSP_HIP(hipMemcpyAsync(st, sh, sizeof(BatchCol) * k, hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipMemcpyAsync(frozen, fh, sizeof(int) * k, hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));  // the pinned mirrors are rewritten by the fetches below
  if (running == 0) return PSP_OK;

  // what the loop can do for all columns at once
  const bool block_product = Acsr != nullptr && w4 != 0;
  const bool batched = fused && (block_product || coop_order);
  // a multigrid K is one block cycle (psp_mg.hip) that reads the device flags itself; with the block product beside it
  // nothing in an iteration depends on the host's view of the flags, and the launches do not depend on k: the cycle's, then
  // r.z, head, pupdate, product, finish, xr, finish
  const bool mg_block = !fused && K && K->kind == PSP_OP_MG && K->mg && mg_block_routed(K->mg);
  const bool mg_batched = mg_block && block_product;
  // launches per iteration where they do not depend on k: pupdate, product (+ its dot in the one-kernel order), finish, xr, finish
  note_solve("pcg_batch", batched ? (coop_order ? 6 : 5) : mg_batched ? mg_launches(K->mg) + 7 : -1,
             batched ? 72 + (dinv ? 16 : 0) : -1, dinv ? 1 : 0);
  const int kBatch = batched || mg_batched ? 16 : 1;  // iterations enqueued between two looks at the states
  int enqueued = 0;
  std::vector<int> live(k);
  for (int c = 0; c < k; ++c) live[c] = !fh[c];
  while (running > 0) {
    const int batch = std::max(1, std::min(kBatch, maxit - enqueued));
    for (int b = 0; b < batch; ++b) {
      const double *zsrc = R;
      if (!fused) {  // z = K r (pcg.c:93-96), rho = r.z (pcg.c:100), then the head of the iteration
        if (K) {
          if (mg_block) {
            PSP_TRY(op_apply_block(K, k, R, n, Z, n, frozen));
          } else {
            for (int c = 0; c < k; ++c)
              if (live[c]) PSP_TRY(op_apply(K, R + (size_t)c * n, Z + (size_t)c * n));
          }
          zsrc = Z;
        }
        hipLaunchKernelGGL(bdot_kernel, vgrid, dim3(kBlock), 0, stream(), (long)n, k, (const double *)R, (long)n, zsrc,
                           (long)n, parts, pstride, (const int *)frozen, 0);
        PSP_LAUNCH_CHECK();
        PSP_TRY(finish_step<kStepHead>(parts, spans, pstride, k, 0, k, st, frozen, 0));
      }
      hipLaunchKernelGGL(bpupdate_kernel, vgrid, dim3(kBlock), 0, stream(), (long)n, zsrc, (long)n, fd, P, (long)n,
                         (const BatchCol *)st, (const int *)frozen);
      PSP_LAUNCH_CHECK();
      // q = A p, p.q (pcg.c:116-117)
      if (coop_order) {  // any block kernel for q, then p.q in the one-kernel loop's order
        PSP_TRY(csr_spmm_launch(Acsr, k, P, n, Q, n, frozen, nullptr, 0, nullptr));
        hipLaunchKernelGGL(bdot_kernel, dim3(cgrid, k), dim3(kBlock), 0, stream(), (long)n, k, (const double *)P, (long)n,
                           (const double *)Q, (long)n, parts, pstride, (const int *)frozen, 1);
        PSP_LAUNCH_CHECK();
        PSP_TRY(finish_step<kStepPq>(parts, cwaves, pstride, k, 0, k, st, frozen, 0, cnwg));
      } else if (block_product) {
        int np = 0;
        PSP_TRY(csr_spmm_launch(Acsr, k, P, n, Q, n, frozen, parts, pstride, &np));
        if (np == 0) return fail(PSP_EINVAL, "psp_pcg_batch: the block product left no p.q partial sums");
        PSP_TRY(finish_step<kStepPq>(parts, np, pstride, k, 0, k, st, frozen, 0));
      } else if (Acsr) {  // another kernel family: its own product, whose fused dot has its own order of partial sums
        for (int c = 0; c < k; ++c) {
          if (!live[c]) continue;
          int np = 0;
          double *pc = P + (size_t)c * n;
          PSP_TRY(csr_spmv_launch_stored(Acsr, pc, Q + (size_t)c * n, pc, w->partials, &np, frozen + c));
          PSP_TRY(finish_step<kStepPq>(w->partials, np, kMaxParts, 1, 0, 1, st + c, frozen + c, 0));
        }
      } else {
        for (int c = 0; c < k; ++c)
          if (live[c]) PSP_TRY(op_apply(A, P + (size_t)c * n, Q + (size_t)c * n));
        hipLaunchKernelGGL(bdot_kernel, vgrid, dim3(kBlock), 0, stream(), (long)n, k, (const double *)P, (long)n,
                           (const double *)Q, (long)n, parts, pstride, (const int *)frozen, 0);
        PSP_LAUNCH_CHECK();
        PSP_TRY(finish_step<kStepPq>(parts, spans, pstride, k, 0, k, st, frozen, 0));
      }
      hipLaunchKernelGGL(bxr_kernel, coop_order ? dim3(cgrid, k) : vgrid, dim3(kBlock), 0, stream(), (long)n, k,
                         (const double *)P, (long)n, (const double *)Q, (long)n, fd, X, ldx, R, (long)n,
                         (const BatchCol *)st, (const int *)frozen, parts, pstride, coop_order ? 1 : 0);
      PSP_LAUNCH_CHECK();
      PSP_TRY(finish_step<kStepXr>(parts, coop_order ? cwaves : spans, pstride, k, 0, k, st, frozen, fused ? 1 : 0,
                                   coop_order ? cnwg : 0));
    }
    enqueued += batch;
    PSP_HIP(hipGetLastError());
    PSP_HIP(hipMemcpyAsync(fh, frozen, sizeof(int) * k, hipMemcpyDeviceToHost, stream()));
    PSP_HIP(hipStreamSynchronize(stream()));
    running = 0;
    for (int c = 0; c < k; ++c) {
      if (live[c] && fh[c]) live[c] = 0;
      running += live[c];
    }
  }
  PSP_HIP(hipMemcpyAsync(sh, st, sizeof(BatchCol) * k, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  for (int c = 0; c < k; ++c) {
    if (decided[c]) continue;  // before the loop
    info[c] = sh[c].info;
    iter[c] = sh[c].iter;
    relres[c] = sh[c].relres;
  }
  return PSP_OK;
}

}  // namespace psp

using namespace psp;

static int batch_args(const psp_op *A, const psp_op *K, int n, int k, const void *X, long ldx, const void *B, long ldb,
                      const int *info, const int *iter, const double *relres) {
  if (!A || !X || !B || !info || !iter || !relres) return fail(PSP_EINVAL, "psp_pcg_batch: NULL argument");
  if (n <= 0) return fail(PSP_EINVAL, "psp_pcg_batch: n must be positive");
  if (k < 1) return fail(PSP_EINVAL, "psp_pcg_batch: k = %d columns (at least one)", k);
  if (A->n != n) return fail(PSP_EINVAL, "psp_pcg_batch: operator order %d != n %d", A->n, n);
  if (K && K->n != n) return fail(PSP_EINVAL, "psp_pcg_batch: preconditioner order %d != n %d", K->n, n);
  if (ldx < n || ldb < n) return fail(PSP_EINVAL, "psp_pcg_batch: leading dimension below n = %d (ldx %ld, ldb %ld)", n, ldx, ldb);
  if ((A->kind == PSP_OP_CSR && A->csr && A->csr->multi) || (K && K->kind == PSP_OP_JACOBI && K->jac && K->jac->multi))
    return fail(PSP_EINVAL, "psp_pcg_batch is not available on a multi-device matrix (psp_csr_*_multi)");
  if (cpu_mode())
    return fail(PSP_ENODEV, "psp_pcg_batch: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  if (n > kMaxN)
    return fail(PSP_EINVAL, "psp_pcg_batch: n = %d is beyond the %d rows whose partial sums one finishing workgroup adds", n, kMaxN);
  return PSP_OK;
}

static int batch_precon_status(const psp_op *K) {
  if (!K || K->kind != PSP_OP_SSOR || !K->ssor) return PSP_OK;
  PSP_HIP(hipStreamSynchronize(stream()));
  return ssor_error_check(K->ssor);
}

extern "C" {

int psp_pcg_batch_dev(const psp_op_t *A, const psp_op_t *K, int n, int k, double *X_dev, long ldx, const double *B_dev,
                      long ldb, double tol, int maxit, int *info, int *iter, double *relres) {
  PSP_API_GUARD_OPS(A, K);
  PSP_TRY(batch_args(A, K, n, k, X_dev, ldx, B_dev, ldb, info, iter, relres));
  PSP_TRY(ensure_device());
  PSP_TRY(pcg_batch_dev(A, K, n, k, X_dev, ldx, B_dev, ldb, tol, maxit, info, iter, relres));
  return batch_precon_status(K);
}

int psp_pcg_batch(const psp_op_t *A, const psp_op_t *K, int n, int k, double *X_host, long ldx, const double *B_host,
                  long ldb, double tol, int maxit, int *info, int *iter, double *relres) {
  PSP_API_GUARD_OPS(A, K);
  PSP_TRY(batch_args(A, K, n, k, X_host, ldx, B_host, ldb, info, iter, relres));
  PSP_TRY(ensure_device());
  const size_t nk = (size_t)n * k;
  double *x = nullptr, *b = nullptr;
  PSP_TRY(scratch_get(nk, &x));
  int rc = scratch_get(nk, &b);
  if (rc == PSP_OK) {
    const size_t row = sizeof(double) * (size_t)n;
    const hipError_t e1 = hipMemcpy2DAsync(x, row, X_host, sizeof(double) * ldx, row, k, hipMemcpyHostToDevice, stream());
    const hipError_t e2 = hipMemcpy2DAsync(b, row, B_host, sizeof(double) * ldb, row, k, hipMemcpyHostToDevice, stream());
    if (e1 != hipSuccess || e2 != hipSuccess) rc = fail(PSP_ENODEV, "psp_pcg_batch: copy to the device failed");
    if (rc == PSP_OK) rc = pcg_batch_dev(A, K, n, k, x, n, b, n, tol, maxit, info, iter, relres);
    if (rc == PSP_OK) {
      const hipError_t e3 = hipMemcpy2DAsync(X_host, sizeof(double) * ldx, x, row, row, k, hipMemcpyDeviceToHost, stream());
      const hipError_t e4 = hipStreamSynchronize(stream());
      if (e3 != hipSuccess || e4 != hipSuccess) rc = fail(PSP_ENODEV, "psp_pcg_batch: copy from the device failed");
    }
    if (rc == PSP_OK) rc = batch_precon_status(K);
  }
  (void)hipStreamSynchronize(stream());
  scratch_put(x, nk);
  scratch_put(b, nk);
  return rc;
}

}  // extern "C"
