// psp_spmm.hip -- products with a block of vectors: Y[:, c] = A X[:, c], c < k, the matrix streamed once per group of up
// to eight columns instead of once per column.  Blocks are column-major as in psp_bvec.hip: column c of X starts at
// X + c*ldx (ldx >= ncols), column c of Y at Y + c*ldy (ldy >= nrows); rows beyond the matrix order and columns >= k are
// never written.
//
//     csr_spmm_w4     handles whose product is csr_spmv_w4 (offset-major value blocks of 128 rows + 16-bit row masks,
//                     read through csr_w4_view): a row pair's values and masks are loaded once, the x pairs of every column
//                     of the group come from clamped addresses with the edge repair of csr_spmv_w4, and each column's
//                     stored products are added left to right under the mask -- column c has the bits of csr_spmv_w4 on
//                     X[:, c].  Workgroup = 512 rows, placed by the XCD stripe of the single-vector launch, so the optional
//                     p.q partial sums (batched PCG) land where csr_spmv_w4's fused dot leaves them.
//                     HBM bytes per row at k columns: 8*NO + 2 (matrix) + 16 k (x once, y once)
//                     against k * (8*NO + 2 + 16) for k single products.
//     csr_spmm_rows   any CSR handle that still has ind / col / val: one wave per 64 consecutive rows walks their
//                     nonzeros in tiles of 128 (col and val read once, coalesced), parks the products of every column in
//                     LDS and lets lane i add row i's products in stored order, carrying the sums from tile to tile -- one
//                     sequential left-to-right sum per row and column (csr_mat.c:49-54), empty rows and rows longer
//                     than any tile included.
//                     HBM bytes per row at k columns: 12 nnz/row + 4 (matrix) + 16 k against k * (12 nnz/row + 20).
// Both use 8-byte-aligned pair accesses for X and Y (the hardware issues them as 16-byte accesses; odd leading dimensions
// need no second form) and are built with -ffp-contract=off like everything else.  No atomics.
#include "psp_internal.h"

namespace psp {
namespace {

typedef double d2v __attribute__((ext_vector_type(2)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

constexpr int kW4Rows = 128;    // rows per value block of the index-free layout (psp_csr_kernels.h kDiaRows)
constexpr int kMaxCols = 8;     // columns whose running sums a thread keeps in registers
constexpr int kRowsTile = 128;  // nonzeros per LDS tile of csr_spmm_rows

struct W4Offs {
  int o[12];
};

// `skip` (batched PCG): column c is neither computed nor written when skip[c] != 0; nullptr: every column.
// partials != nullptr: partials[c*pstride + blockIdx.x] = sum over the workgroup's rows of X[r, c] * Y[r, c] in the
// order of csr_spmv_w4's fused dot (pair per lane, wave tree, the four waves left to right).
template <int NO, int KC>
__global__ __launch_bounds__(256) void csr_spmm_w4(int nblk, int nrows, int ncols, int stripe, W4Offs offs,
                                                   const double *__restrict__ valT,
                                                   const unsigned short *__restrict__ mask, int k,
                                                   const double *__restrict__ X, long ldx, double *__restrict__ Y,
                                                   long ldy, const int *__restrict__ skip,
                                                   double *__restrict__ partials, long pstride) {
  __shared__ double red[4][KC];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = blockIdx.y * kMaxCols;
  const int cnt = min(KC, k - c0);
  int vb = (int)blockIdx.x;  // XCD-aware placement, as csr_spmv_w4
  if (stripe > 0) {
    const int q = vb >> 3;
    vb = ((q / stripe) * 8 + (vb & 7)) * stripe + q % stripe;
  }
  const int blk = vb * 4 + wid;
  const long r = (long)blk * kW4Rows + 2 * lane;
  double dsum[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) dsum[c] = 0.0;
  if (blk < nblk && r < nrows) {
    const unsigned mm = *reinterpret_cast<const unsigned *>(mask + r);  // padded to a whole block
    const unsigned m0 = mm & 0xffffu, m1 = mm >> 16;
    const double *vp = valT + (size_t)blk * NO * kW4Rows + 2 * lane;
    d2v v[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) v[o] = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(vp + o * kW4Rows));
    const long cmax = (long)ncols - 2;  // ncols >= 2
    long cc[NO];
    bool edge = false;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const long c = r + offs.o[o];
      cc[o] = c < 0 ? 0 : (c > cmax ? cmax : c);
      edge |= cc[o] != c;
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      if (c >= cnt) continue;
      if (skip && skip[c0 + c]) continue;
      const double *__restrict__ x = X + (size_t)(c0 + c) * ldx;
      double *__restrict__ y = Y + (size_t)(c0 + c) * ldy;
      d2v xv[NO];
#pragma unroll
      for (int o = 0; o < NO; ++o) {  // unconditional loads from clamped addresses ...
        const d2u t = *reinterpret_cast<const d2u *>(x + cc[o]);
        xv[o].x = t.x;
        xv[o].y = t.y;
      }
      if (edge) {  // ... repaired by the lanes at the two ends of x
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          const long cl = r + offs.o[o];
          if (cl < 0 || cl > cmax) {
            xv[o].x = (cl >= 0 && cl < ncols) ? x[cl] : 0.0;
            xv[o].y = (cl + 1 >= 0 && cl + 1 < ncols) ? x[cl + 1] : 0.0;
          }
        }
      }
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const double t0 = a0 + v[o].x * xv[o].x;
        const double t1 = a1 + v[o].y * xv[o].y;
        a0 = ((m0 >> o) & 1u) ? t0 : a0;
        a1 = ((m1 >> o) & 1u) ? t1 : a1;
      }
      if (r + 1 < nrows) {
        d2u outu;
        outu.x = a0;
        outu.y = a1;
        __builtin_nontemporal_store(outu, reinterpret_cast<d2u *>(y + r));
        if (partials) {
          const d2u u = *reinterpret_cast<const d2u *>(x + r);
          dsum[c] += u.x * a0;
          dsum[c] += u.y * a1;
        }
      } else {
        y[r] = a0;
        if (partials) dsum[c] += x[r] * a0;
      }
    }
  }
  if (partials) {
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const double s = psp_wave_sum(dsum[c]);
      if (lane == 0) red[wid][c] = s;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < cnt && (!skip || !skip[c0 + c]))
      partials[(size_t)(c0 + c) * pstride + blockIdx.x] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  }
}

// One wave (= one workgroup) per 64 consecutive rows.  prod[c][j]: the product of the tile's j-th nonzero with column c.
template <int KC>
__global__ __launch_bounds__(64) void csr_spmm_rows(int nrows, const int *__restrict__ ind, const int *__restrict__ col,
                                                    const double *__restrict__ val, int k, const double *__restrict__ X,
                                                    long ldx, double *__restrict__ Y, long ldy,
                                                    const int *__restrict__ skip) {
  __shared__ double prod[KC][kRowsTile];
  const int lane = threadIdx.x;
  const int c0 = blockIdx.y * kMaxCols;
  const int cnt = min(KC, k - c0);
  const long row0 = (long)blockIdx.x * 64;
  const long rlast = row0 + 64 < nrows ? row0 + 64 : nrows;
  const long r = row0 + lane;
  const int kbeg = ind[row0], kend = ind[rlast];  // the wave's nonzeros (uniform)
  int lo = 0, hi = 0;
  if (r < nrows) {
    lo = ind[r];
    hi = ind[r + 1];
  }
  double acc[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) acc[c] = 0.0;
  for (int t0 = kbeg; t0 < kend; t0 += kRowsTile) {
#pragma unroll
    for (int u = 0; u < kRowsTile / 64; ++u) {
      const int j = u * 64 + lane;
      const int kk = t0 + j;
      if (kk < kend) {
        const int cj = col[kk];
        const double vj = val[kk];
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (c < cnt) prod[c][j] = vj * X[(size_t)(c0 + c) * ldx + cj];
      }
    }
    __syncthreads();
    const int a = (lo > t0 ? lo : t0) - t0;
    const int b = (hi < t0 + kRowsTile ? hi : t0 + kRowsTile) - t0;
    for (int j = a; j < b; ++j) {
#pragma unroll
      for (int c = 0; c < KC; ++c)
        if (c < cnt) acc[c] += prod[c][j];
    }
    __syncthreads();
  }
  if (r < nrows) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < cnt && (!skip || !skip[c0 + c])) Y[(size_t)(c0 + c) * ldy + r] = acc[c];
  }
}

// Y[:, c] = X[:, c] .* dinv (jacobi_first_kernel's product), every column in one launch; thread t owns rows 2t, 2t+1
__global__ __launch_bounds__(256) void jacobi_block_kernel(long n, int k, const double *__restrict__ dinv,
                                                           const double *__restrict__ X, long ldx,
                                                           double *__restrict__ Y, long ldy) {
  for (long base = (long)blockIdx.x * kVecSpan; base < n; base += (long)gridDim.x * kVecSpan) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long i = base + 2 * threadIdx.x + u;
      if (i >= n) continue;
      const double d = dinv[i];
      for (int c = 0; c < k; ++c) Y[(size_t)c * ldy + i] = X[(size_t)c * ldx + i] * d;
    }
  }
}

template <int NO>
int launch_spmm_w4(const psp_csr *A, const W4View &v, int k, const double *X, long ldx, double *Y, long ldy,
                   const int *skip, double *partials, long pstride) {
  const int nblk = (A->nrows + kW4Rows - 1) / kW4Rows;
  W4Offs offs;
  for (int i = 0; i < 12; ++i) offs.o[i] = v.offs[i];
  const int groups = (k + kMaxCols - 1) / kMaxCols;
#define PSP_SPMM_W4(KC)                                                                                              \
  hipLaunchKernelGGL((csr_spmm_w4<NO, KC>), dim3(v.grid, groups), dim3(256), 0, stream(), nblk, A->nrows, A->ncols,  \
                     v.stripe, offs, v.valT, v.mask, k, X, ldx, Y, ldy, skip, partials, pstride)
  if (k == 1) PSP_SPMM_W4(1);
  else if (k == 2) PSP_SPMM_W4(2);
  else if (k <= 4) PSP_SPMM_W4(4);
  else PSP_SPMM_W4(8);
#undef PSP_SPMM_W4
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int launch_spmm_rows(const psp_csr *A, int k, const double *X, long ldx, double *Y, long ldy, const int *skip) {
  const int grid = (A->nrows + 63) / 64;
  const int groups = (k + kMaxCols - 1) / kMaxCols;
#define PSP_SPMM_ROWS(KC)                                                                                          \
  hipLaunchKernelGGL((csr_spmm_rows<KC>), dim3(grid, groups), dim3(64), 0, stream(), A->nrows, A->ind, A->col, A->val, \
                     k, X, ldx, Y, ldy, skip)
  if (k == 1) PSP_SPMM_ROWS(1);
  else if (k == 2) PSP_SPMM_ROWS(2);
  else if (k <= 4) PSP_SPMM_ROWS(4);
  else PSP_SPMM_ROWS(8);
#undef PSP_SPMM_ROWS
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

}  // namespace

static bool ranges_overlap(const double *a, size_t na, const double *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + sizeof(double) * na, b0 = (uintptr_t)b, b1 = b0 + sizeof(double) * nb;
  return a0 < b1 && b0 < a1;
}

int block_args(const char *what, int nrows, int ncols, int k, const double *X, long ldx, const double *Y, long ldy) {
  if (k < 1) return fail(PSP_EINVAL, "%s: k = %d columns (at least one)", what, k);
  if (!X || !Y) return fail(PSP_EINVAL, "%s: NULL argument", what);
  if (ldx < ncols) return fail(PSP_EINVAL, "%s: ldx = %ld is below the %d rows of X", what, ldx, ncols);
  if (ldy < nrows) return fail(PSP_EINVAL, "%s: ldy = %ld is below the %d rows of Y", what, ldy, nrows);
  if (nrows > 0 && ncols > 0 &&
      ranges_overlap(X, (size_t)(k - 1) * ldx + ncols, Y, (size_t)(k - 1) * ldy + nrows))
    return fail(PSP_EINVAL, "%s: X and Y overlap", what);
  return PSP_OK;
}

int csr_spmm_check(const char *what, const psp_csr *A) {
  if (!A) return fail(PSP_EINVAL, "%s: NULL handle", what);
  if (A->host || cpu_mode())
    return fail(PSP_ENODEV, "%s: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)", what);
  if (A->multi) return fail(PSP_EINVAL, "%s is not available on a multi-device matrix (psp_csr_*_multi)", what);
  if (A->nparts > 0) return fail(PSP_EINVAL, "%s is not available on a matrix that is stored in parts (more than 2^31 - 8192 nonzeros)", what);
  return PSP_OK;
}

// the block product at its device-pointer level (handles locked, arguments checked by the caller).  partials != nullptr
// asks for the p.q partial sums of every column in the order of the single-vector product's fused dot; *nparts = 0 says
// that this handle's product leaves them in an order the block kernels do not reproduce (nothing was written to them).
int csr_spmm_launch(const psp_csr *A, int k, const double *X, long ldx, double *Y, long ldy, const int *skip,
                    double *partials, long pstride, int *nparts) {
  if (nparts) *nparts = 0;
  if (A->nrows == 0) return PSP_OK;
  W4View v;
  int w4 = 0;
  PSP_TRY(csr_w4_view(A, &v, &w4));
  if (w4) {
    // the fused dot is csr_spmv_w4's only where the single product IS csr_spmv_w4 / sss_spmv_w4 (same workgroups, same order)
    if (partials && v.grid > pstride) partials = nullptr;
    int rc = PSP_OK;
    switch (v.no) {
      case 1: rc = launch_spmm_w4<1>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 2: rc = launch_spmm_w4<2>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 3: rc = launch_spmm_w4<3>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 4: rc = launch_spmm_w4<4>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 5: rc = launch_spmm_w4<5>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 6: rc = launch_spmm_w4<6>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 7: rc = launch_spmm_w4<7>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 8: rc = launch_spmm_w4<8>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      case 9: rc = launch_spmm_w4<9>(A, v, k, X, ldx, Y, ldy, skip, partials, pstride); break;
      default: return fail(PSP_EINVAL, "csr_spmm_w4: %d offsets", v.no);
    }
    if (rc == PSP_OK && partials && nparts) *nparts = v.grid;
    return rc;
  }
  if (!A->ind || !A->col || !A->val)
    return fail(PSP_EINVAL, "block product: this handle gave up its CSR arrays and its index-free layout has more than 9 "
                            "offsets (csr_spmv_w4 with 32- / 64-bit masks has no block form)");
  return launch_spmm_rows(A, k, X, ldx, Y, ldy, skip);
}

int jacobi_block_dev(const psp_jacobi *K, int k, const double *X, long ldx, double *Y, long ldy) {
  Workspace *w;
  PSP_TRY(workspace(&w));
  hipLaunchKernelGGL(jacobi_block_kernel, dim3(vec_grid(*w, K->n)), dim3(256), 0, stream(), (long)K->n, k, K->dinv, X, ldx,
                     Y, ldy);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int op_apply_block(const psp_op *op, int k, const double *X, long ldx, double *Y, long ldy, const int *frozen) {
  if (op->kind == PSP_OP_CSR || op->kind == PSP_OP_SSS) {
    const psp_csr *A = op_native_csr(op);
    PSP_TRY(csr_spmm_check("op_apply_block", A));
    return csr_spmm_launch(A, k, X, ldx, Y, ldy, nullptr, nullptr, 0, nullptr);
  }
  if (op->kind == PSP_OP_JACOBI && op->jac && op->jac->steps == 1 && !op->jac->multi && !op->jac->host)
    return jacobi_block_dev(op->jac, k, X, ldx, Y, ldy);
  if (op->kind == PSP_OP_MG && op->mg && mg_block_routed(op->mg)) return mg_apply_block_dev(op->mg, k, X, ldx, Y, ldy, frozen);
  for (int c = 0; c < k; ++c) PSP_TRY(op_apply(op, X + (size_t)c * ldx, Y + (size_t)c * ldy));
  return PSP_OK;
}

}  // namespace psp

using namespace psp;

namespace {

// host blocks through device blocks of leading dimension n (scratch pool)
struct StagedBlocks {
  double *x = nullptr, *y = nullptr;
  size_t nx = 0, ny = 0;
  ~StagedBlocks() {
    scratch_put(x, nx);
    scratch_put(y, ny);
  }
};

int matmat_host(psp_csr *A, const char *what, int k, const double *X_host, long ldx, double *Y_host, long ldy) {
  PSP_TRY(csr_spmm_check(what, A));
  PSP_TRY(block_args(what, A->nrows, A->ncols, k, X_host, ldx, Y_host, ldy));
  PSP_TRY(ensure_device());
  if (A->nrows == 0) return PSP_OK;
  StagedBlocks s;
  s.nx = (size_t)k * A->ncols;
  s.ny = (size_t)k * A->nrows;
  PSP_TRY(scratch_get(s.nx, &s.x));
  PSP_TRY(scratch_get(s.ny, &s.y));
  if (A->ncols > 0)
    PSP_HIP(hipMemcpy2DAsync(s.x, sizeof(double) * A->ncols, X_host, sizeof(double) * ldx, sizeof(double) * A->ncols, k,
                             hipMemcpyHostToDevice, stream()));
  PSP_TRY(csr_spmm_launch(A, k, s.x, A->ncols, s.y, A->nrows, nullptr, nullptr, 0, nullptr));
  PSP_HIP(hipMemcpy2DAsync(Y_host, sizeof(double) * ldy, s.y, sizeof(double) * A->nrows, sizeof(double) * A->nrows, k,
                           hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

int matmat_dev(psp_csr *A, const char *what, int k, const double *X, long ldx, double *Y, long ldy) {
  PSP_TRY(csr_spmm_check(what, A));
  PSP_TRY(block_args(what, A->nrows, A->ncols, k, X, ldx, Y, ldy));
  PSP_TRY(ensure_device());
  return csr_spmm_launch(A, k, X, ldx, Y, ldy, nullptr, nullptr, 0, nullptr);
}

}  // namespace

extern "C" {

int psp_csr_matmat(psp_csr_t *A, int k, const double *X_host, long ldx, double *Y_host, long ldy) {
  PSP_API_GUARD_H(A);
  return matmat_host(A, "psp_csr_matmat", k, X_host, ldx, Y_host, ldy);
}

int psp_csr_matmat_dev(psp_csr_t *A, int k, const double *X_dev, long ldx, double *Y_dev, long ldy) {
  PSP_API_GUARD_H(A);
  return matmat_dev(A, "psp_csr_matmat_dev", k, X_dev, ldx, Y_dev, ldy);
}

int psp_sss_matmat(psp_sss_t *S, int k, const double *X_host, long ldx, double *Y_host, long ldy) {
  PSP_API_GUARD_H(S, S ? S->full : nullptr);
  if (!S) return fail(PSP_EINVAL, "psp_sss_matmat: NULL handle");
  if (S->host || cpu_mode())
    return fail(PSP_ENODEV, "psp_sss_matmat: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  return matmat_host(S->full, "psp_sss_matmat", k, X_host, ldx, Y_host, ldy);
}

int psp_sss_matmat_dev(psp_sss_t *S, int k, const double *X_dev, long ldx, double *Y_dev, long ldy) {
  PSP_API_GUARD_H(S, S ? S->full : nullptr);
  if (!S) return fail(PSP_EINVAL, "psp_sss_matmat_dev: NULL handle");
  if (S->host || cpu_mode())
    return fail(PSP_ENODEV, "psp_sss_matmat_dev: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  return matmat_dev(S->full, "psp_sss_matmat_dev", k, X_dev, ldx, Y_dev, ldy);
}

int psp_op_apply_block_dev(const psp_op_t *op, int k, const double *X_dev, long ldx, double *Y_dev, long ldy) {
  PSP_API_GUARD_OPS(op, nullptr);
  if (!op) return fail(PSP_EINVAL, "psp_op_apply_block_dev: NULL operator");
  if (cpu_mode())
    return fail(PSP_ENODEV, "psp_op_apply_block_dev: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  PSP_TRY(block_args("psp_op_apply_block_dev", op->n, op->n, k, X_dev, ldx, Y_dev, ldy));
  PSP_TRY(ensure_device());
  return op_apply_block(op, k, X_dev, ldx, Y_dev, ldy);
}

}  // extern "C"
