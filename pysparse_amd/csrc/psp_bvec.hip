// psp_bvec.hip -- tall-skinny dense algebra on n x m column-major blocks (m: a few dozen columns), the inner work of the
// Jacobi-Davidson eigensolver beside its products (psp_jdsym.hip; the dgemv / dgemm calls of jdsym.c, orthopack.c and
// correq.c in the reference):
//     tdot    h = V' x            one pass over V, x read once per group of kTdotCols columns, fixed-order partial sums
//     gemv    y = beta y + alpha V h   (q = V u, x -= V h), h read from the device
//     rotate  V[:, dst0 .. dst0+jn) = V[:, 0 .. j) U[:, u0 .. u0+jn)  in place, row by row
// and of the block eigensolver (psp_lobpcg.hip):
//     gram    G = A' B            a thread keeps an 8 x 4 tile of sums; column b has tdot's bits on B[:, b]
//     resid   R[:, slot[c]] = AX[:, c] - theta[c] MX[:, c] and r . r per column, one pass
// All of them move far more bytes than they do arithmetic (the rotate at j = 25 -> 10 does ~2 flop per byte): fp64 vector
// arithmetic, no MFMA.  Column c starts at V + c*ld, ld >= n; rows n..ld are never touched.  tdot and gemv use 16-byte
// accesses when n is even and every column start is 16-byte aligned (ld even), 8-byte ones otherwise -- the same rounded
// operations in the same order either way.  The rotate always uses 8-byte accesses (one row per lane: a wave reads 512
// contiguous bytes per column) and one wave per workgroup with 512 j bytes of LDS, which bounds its occupancy; it runs
// at restarts and after convergence only, not inside the inner solves.
// Grids: one workgroup per 512 rows up to 65 536 workgroups, i.e. the loops over spans in tdot / gemv run more than once
// only beyond n = 2^25 -- a size no test reaches.
// Vector-at-a-time (k_dot / axpy per column) an orthogonalisation against m columns streams 3*8*n*m bytes in 2m launches;
// here 8*n*(m+1) + 8*n*(m+2) bytes in three.
#include "psp_internal.h"

namespace psp {
namespace {

constexpr int kBvBlock = 256;
constexpr int kBvSpan = 512;      // rows per workgroup pass: one 16-byte access per lane and column
constexpr int kTdotCols = 8;      // columns whose running sums a thread keeps in registers
constexpr int kBvMaxParts = 256 * kOneBlockGroups;  // what ONE finishing block adds in the canonical order (psp_internal.h)
constexpr int kRotRows = 64;      // rows per workgroup of the rotate: the row block waits in LDS
constexpr int kRotMaxJ = 128;
constexpr int kRotOut = 4;        // output columns per pass over a row's LDS copy
constexpr int kGramTA = 8;        // gram: columns of A x columns of B whose sums a thread keeps in registers
constexpr int kGramTB = 4;
constexpr long kGramPartsCap = 1L << 25;  // gram: partial sums per launch pair (256 MB); more columns of B take further pairs
constexpr int kResidMaxCols = 32;

// per thread: the partial sums of tdot (m columns x grid) and the device copy of the rotate's U, on the device and for
// the stream the thread used last.  Both are consumed in stream order by the call that fills them, so one set per thread
// is enough as long as the thread stays on one stream; when it changes device or stream the old set is let go after the
// device it lives on has drained.  psp_trim() releases the calling thread's set (bv_trim); a thread that ends without
// calling it leaves its set (m * ceil(n / 512) doubles + 128 KiB) allocated until the process ends.
struct BvScratch {
  int device = -1;
  hipStream_t last = nullptr;
  double *parts = nullptr;
  size_t parts_cap = 0;
  double *U = nullptr;
};
thread_local BvScratch tl_bv;

void bv_release(BvScratch &s) {
  if (s.parts || s.U) {
    int cur = -1;
    const bool moved = s.device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != s.device;
    if (moved) (void)hipSetDevice(s.device);
    (void)hipDeviceSynchronize();
    if (s.parts) (void)hipFree(s.parts);
    if (s.U) (void)hipFree(s.U);
    if (moved) (void)hipSetDevice(cur);
    (void)hipGetLastError();
  }
  s = BvScratch();
}

int bv_scratch(size_t parts_needed, BvScratch **out) {
  PSP_TRY(ensure_device());
  BvScratch &s = tl_bv;
  const int d = current_device();
  if (s.device != d || s.last != stream()) {
    bv_release(s);
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
    size_t cap = parts_needed < 4096 ? 4096 : parts_needed;
    PSP_HIP(hipMalloc((void **)&s.parts, sizeof(double) * cap));
    s.parts_cap = cap;
  }
  *out = &s;
  return PSP_OK;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// h partial sums: workgroup b adds rows [b*span, ...) in steps of gridDim.x*span; lane order inside a wave, then the four
// waves in order: parts[c*pstride + b].  VEC: rows 2t, 2t+1 of a span per thread (one double2 per column), else rows t, t+256
template <bool VEC>
__global__ __launch_bounds__(kBvBlock) void bv_tdot_kernel(long n, int m, const double *__restrict__ V, long ld,
                                                           const double *__restrict__ x, double *__restrict__ parts,
                                                           long pstride) {
  __shared__ double sh[kBvBlock / 64][kTdotCols];
  const int c0 = blockIdx.y * kTdotCols;
  const int cnt = min(kTdotCols, m - c0);
  const double *__restrict__ Vg = V + (size_t)c0 * ld;
  double acc[kTdotCols];
#pragma unroll
  for (int c = 0; c < kTdotCols; ++c) acc[c] = 0.0;
  for (long base = (long)blockIdx.x * kBvSpan; base < n; base += (long)gridDim.x * kBvSpan) {
    if constexpr (VEC) {
      const long i = base + 2 * threadIdx.x;  // n is even in this form
      if (i < n) {
        const double2 xx = *reinterpret_cast<const double2 *>(x + i);
        double2 vv[kTdotCols];
#pragma unroll
        for (int c = 0; c < kTdotCols; ++c)
          if (c < cnt) vv[c] = *reinterpret_cast<const double2 *>(Vg + (size_t)c * ld + i);
#pragma unroll
        for (int c = 0; c < kTdotCols; ++c)
          if (c < cnt) {
            acc[c] += vv[c].x * xx.x;
            acc[c] += vv[c].y * xx.y;
          }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long i = base + threadIdx.x + u * kBvBlock;
        if (i < n) {
          const double xx = x[i];
          double vv[kTdotCols];
#pragma unroll
          for (int c = 0; c < kTdotCols; ++c)
            if (c < cnt) vv[c] = Vg[(size_t)c * ld + i];
#pragma unroll
          for (int c = 0; c < kTdotCols; ++c)
            if (c < cnt) acc[c] += vv[c] * xx;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kTdotCols; ++c) {
    const double s = psp_wave_sum(acc[c]);
    if (lane == 0) sh[wid][c] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < cnt) {
    double s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBvBlock / 64; ++w) s += sh[w][threadIdx.x];
    parts[(size_t)(c0 + threadIdx.x) * pstride + blockIdx.x] = s;
  }
}

// h[c] = reduce(parts[c*pstride .. + nparts)) in the canonical order of psp_internal.h: one workgroup per column
__global__ __launch_bounds__(kReduceBlock) void bv_tdot_finish_kernel(const double *__restrict__ parts, int nparts,
                                                                      long pstride, double *__restrict__ h) {
  __shared__ double sh[kOneBlockGroups];
  reduce_block(parts + (size_t)blockIdx.x * pstride, nparts, 1, 0, true, h + blockIdx.x, sh);
}

// y[i] = beta*y[i] + alpha * (V[i,0] h[0] + V[i,1] h[1] + ...), left to right from 0.0; BETA0: y is not read.
// h[c] is uniform over the wave: the compiler reads it through the scalar cache.
template <bool VEC, bool BETA0>
__global__ __launch_bounds__(kBvBlock) void bv_gemv_kernel(long n, int m, const double *__restrict__ V, long ld,
                                                           const double *__restrict__ h, double alpha, double beta,
                                                           double *__restrict__ y) {
  constexpr int W = VEC ? 2 : 1;
  constexpr int kUnroll = 8;
  for (long base = (long)blockIdx.x * kBvSpan; base < n; base += (long)gridDim.x * kBvSpan) {
#pragma unroll
    for (int u = 0; u < (VEC ? 1 : 2); ++u) {
      const long i = VEC ? base + 2 * threadIdx.x : base + threadIdx.x + u * kBvBlock;
      if (i >= n) continue;
      double s[W];
#pragma unroll
      for (int e = 0; e < W; ++e) s[e] = 0.0;
      int c = 0;
      for (; c + kUnroll <= m; c += kUnroll) {
        double vv[kUnroll][W];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
          const double *p = V + (size_t)(c + k) * ld + i;
          if constexpr (VEC) {
            const double2 t = *reinterpret_cast<const double2 *>(p);
            vv[k][0] = t.x;
            vv[k][1] = t.y;
          } else {
            vv[k][0] = *p;
          }
        }
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
          const double hc = h[c + k];
#pragma unroll
          for (int e = 0; e < W; ++e) s[e] += vv[k][e] * hc;
        }
      }
      for (; c < m; ++c) {
        const double hc = h[c];
        const double *p = V + (size_t)c * ld + i;
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] += p[e] * hc;
      }
      double out[W];
#pragma unroll
      for (int e = 0; e < W; ++e) {
        if constexpr (BETA0)
          out[e] = alpha * s[e];
        else
          out[e] = beta * y[i + e] + alpha * s[e];
      }
      if constexpr (VEC)
        *reinterpret_cast<double2 *>(y + i) = double2{out[0], out[1]};
      else
        y[i] = out[0];
    }
  }
}

// One row per thread: the row's j entries go to LDS (tile[c*kRotRows + t]: each thread reads back only what it wrote, so
// the copy needs no barrier and has no bank conflicts), then kRotOut results at a time are formed left to right and
// written.  Every read of the row precedes every write of it: source and destination columns may overlap.
// Uc: the jn columns of U that are used, compact (j x jn), on the device -- uniform addresses, scalar cache.
__global__ __launch_bounds__(kRotRows) void bv_rotate_kernel(long n, int j, double *__restrict__ V, long ld,
                                                             const double *__restrict__ Uc, int jn, int dst0) {
  extern __shared__ double tile[];
  const long i = (long)blockIdx.x * kRotRows + threadIdx.x;
  if (i >= n) return;
  double *row = tile + threadIdx.x;
  for (int c = 0; c < j; ++c) row[(size_t)c * kRotRows] = V[(size_t)c * ld + i];
  for (int o = 0; o < jn; o += kRotOut) {
    double acc[kRotOut];
#pragma unroll
    for (int e = 0; e < kRotOut; ++e) acc[e] = 0.0;
    const int no = min(kRotOut, jn - o);
    for (int c = 0; c < j; ++c) {
      const double v = row[(size_t)c * kRotRows];
#pragma unroll
      for (int e = 0; e < kRotOut; ++e)
        if (e < no) acc[e] += v * Uc[(size_t)(o + e) * j + c];
    }
#pragma unroll
    for (int e = 0; e < kRotOut; ++e)
      if (e < no) V[(size_t)(dst0 + o + e) * ld + i] = acc[e];
  }
}

// G = A' B partial sums: the workgroup adds its 512-row spans for a kGramTA x kGramTB tile of (column of A, column of B)
// pairs in registers -- an element of A is used kGramTB times, one of B kGramTA times.  Rows go to lanes, lanes to waves
// and waves to the workgroup's sum exactly as in bv_tdot_kernel with V = A and x = one column of B, so entry (a, b) has
// the bits of that kernel's partial sum.  parts[(b*ma + a)*pstride + blockIdx.x], b counted from the first column given.
template <bool VEC>
__global__ __launch_bounds__(kBvBlock) void bv_gram_kernel(long n, int ma, const double *__restrict__ A, long lda, int mb,
                                                           const double *__restrict__ B, long ldb,
                                                           double *__restrict__ parts, long pstride) {
  __shared__ double sh[kBvBlock / 64][kGramTA * kGramTB];
  const int a0 = blockIdx.y * kGramTA, b0 = blockIdx.z * kGramTB;
  const int ca = min(kGramTA, ma - a0), cb = min(kGramTB, mb - b0);
  const double *__restrict__ Ag = A + (size_t)a0 * lda;
  const double *__restrict__ Bg = B + (size_t)b0 * ldb;
  double acc[kGramTA][kGramTB];
#pragma unroll
  for (int a = 0; a < kGramTA; ++a)
#pragma unroll
    for (int b = 0; b < kGramTB; ++b) acc[a][b] = 0.0;
  for (long base = (long)blockIdx.x * kBvSpan; base < n; base += (long)gridDim.x * kBvSpan) {
    if constexpr (VEC) {
      const long i = base + 2 * threadIdx.x;  // n is even in this form
      if (i < n) {
        double2 aa[kGramTA], bb[kGramTB];
#pragma unroll
        for (int b = 0; b < kGramTB; ++b)
          bb[b] = b < cb ? *reinterpret_cast<const double2 *>(Bg + (size_t)b * ldb + i) : double2{0.0, 0.0};
#pragma unroll
        for (int a = 0; a < kGramTA; ++a)
          aa[a] = a < ca ? *reinterpret_cast<const double2 *>(Ag + (size_t)a * lda + i) : double2{0.0, 0.0};
#pragma unroll
        for (int a = 0; a < kGramTA; ++a)
#pragma unroll
          for (int b = 0; b < kGramTB; ++b) {
            acc[a][b] += aa[a].x * bb[b].x;
            acc[a][b] += aa[a].y * bb[b].y;
          }
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long i = base + threadIdx.x + u * kBvBlock;
        if (i < n) {
          double aa[kGramTA], bb[kGramTB];
#pragma unroll
          for (int b = 0; b < kGramTB; ++b) bb[b] = b < cb ? Bg[(size_t)b * ldb + i] : 0.0;
#pragma unroll
          for (int a = 0; a < kGramTA; ++a) aa[a] = a < ca ? Ag[(size_t)a * lda + i] : 0.0;
#pragma unroll
          for (int a = 0; a < kGramTA; ++a)
#pragma unroll
            for (int b = 0; b < kGramTB; ++b) acc[a][b] += aa[a] * bb[b];
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < kGramTA; ++a)
#pragma unroll
    for (int b = 0; b < kGramTB; ++b) {
      const double s = psp_wave_sum(acc[a][b]);
      if (lane == 0) sh[wid][a * kGramTB + b] = s;
    }
  __syncthreads();
  if ((int)threadIdx.x < kGramTA * kGramTB) {
    const int a = threadIdx.x / kGramTB, b = threadIdx.x % kGramTB;
    if (a < ca && b < cb) {
      double s = sh[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kBvBlock / 64; ++w) s += sh[w][threadIdx.x];
      parts[((size_t)(b0 + b) * ma + (a0 + a)) * pstride + blockIdx.x] = s;
    }
  }
}

// G[a + b*ldg] = reduce(parts of entry b*ma + a) in the canonical order: one workgroup per entry
__global__ __launch_bounds__(kReduceBlock) void bv_gram_finish_kernel(const double *__restrict__ parts, int nparts,
                                                                      long pstride, int ma, double *__restrict__ G, long ldg) {
  __shared__ double sh[kOneBlockGroups];
  const int a = blockIdx.x % ma, b = blockIdx.x / ma;
  reduce_block(parts + (size_t)blockIdx.x * pstride, nparts, 1, 0, true, G + (size_t)b * ldg + a, sh);
}

struct BvSlots {  // where column c of the residual block goes (-1: nowhere)
  int s[kResidMaxCols];
};

// r = AX[:, c] - theta[c] * MX[:, c] (product rounded, then the difference), stored at R[:, slot[c]] when slot[c] >= 0,
// and the partial sums of r . r as bv_tdot_kernel forms them for one column (PAIR: rows 2t, 2t + 1, else t, t + 256).
// VLOAD (PAIR only): every column of the three blocks starts on 16 bytes.  blockIdx.y = c.
template <bool PAIR, bool VLOAD>
__global__ __launch_bounds__(kBvBlock) void bv_resid_kernel(long n, const double *__restrict__ AX, long ldax,
                                                            const double *MX, long ldmx,
                                                            const double *__restrict__ theta, BvSlots slots,
                                                            double *R, long ldr, double *__restrict__ parts,
                                                            long pstride) {
  __shared__ double sh[kBvBlock / 64];
  const int c = blockIdx.y;
  const double th = theta[c];
  const int slot = slots.s[c];
  const double *ax = AX + (size_t)c * ldax;
  const double *mx = MX + (size_t)c * ldmx;
  double *r = slot >= 0 ? R + (size_t)slot * ldr : nullptr;
  double acc = 0.0;
  for (long base = (long)blockIdx.x * kBvSpan; base < n; base += (long)gridDim.x * kBvSpan) {
    if constexpr (PAIR) {
      const long i = base + 2 * threadIdx.x;  // n is even in this form
      if (i < n) {
        double a0, a1, m0, m1;
        if constexpr (VLOAD) {
          const double2 av = *reinterpret_cast<const double2 *>(ax + i), mv = *reinterpret_cast<const double2 *>(mx + i);
          a0 = av.x, a1 = av.y, m0 = mv.x, m1 = mv.y;
        } else {
          a0 = ax[i], a1 = ax[i + 1], m0 = mx[i], m1 = mx[i + 1];
        }
        const double p0 = th * m0, p1 = th * m1;
        const double r0 = a0 - p0, r1 = a1 - p1;
        if (r) {
          if constexpr (VLOAD) {
            *reinterpret_cast<double2 *>(r + i) = double2{r0, r1};
          } else {
            r[i] = r0;
            r[i + 1] = r1;
          }
        }
        acc += r0 * r0;
        acc += r1 * r1;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long i = base + threadIdx.x + u * kBvBlock;
        if (i < n) {
          const double p = th * mx[i];
          const double rr = ax[i] - p;
          if (r) r[i] = rr;
          acc += rr * rr;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double s = psp_wave_sum(acc);
  if (lane == 0) sh[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sh[0];
#pragma unroll
    for (int w = 1; w < kBvBlock / 64; ++w) t += sh[w];
    parts[(size_t)c * pstride + blockIdx.x] = t;
  }
}

int bv_grid(long n) {
  long want = (n + kBvSpan - 1) / kBvSpan;
  if (want < 1) want = 1;
  return (int)(want < kBvMaxParts ? want : kBvMaxParts);
}

}  // namespace

void bv_trim() { bv_release(tl_bv); }

int bv_gram(long n, int ma, const double *A, long lda, int mb, const double *B, long ldb, double *G_dev, long ldg) {
  if (ma <= 0 || mb <= 0) return PSP_OK;
  if (n <= 0) {
    PSP_HIP(hipMemset2DAsync(G_dev, sizeof(double) * ldg, 0, sizeof(double) * ma, mb, stream()));
    return PSP_OK;
  }
  const int grid = bv_grid(n);
  // columns of B per launch pair: the partial sums of ma * nb entries stay below kGramPartsCap doubles
  long nb = kGramPartsCap / ((long)ma * grid);
  if (nb >= kGramTB) nb -= nb % kGramTB;
  if (nb < 1) nb = 1;
  if (nb > mb) nb = mb;
  BvScratch *s;
  PSP_TRY(bv_scratch((size_t)ma * nb * grid, &s));
  const bool vec = (n % 2 == 0) && (lda % 2 == 0) && (ldb % 2 == 0) && aligned16(A) && aligned16(B);
  for (int b0 = 0; b0 < mb; b0 += (int)nb) {
    const int cnt = std::min((int)nb, mb - b0);
    const dim3 g(grid, (ma + kGramTA - 1) / kGramTA, (cnt + kGramTB - 1) / kGramTB);
    const double *Bb = B + (size_t)b0 * ldb;
    if (vec)
      hipLaunchKernelGGL(bv_gram_kernel<true>, g, dim3(kBvBlock), 0, stream(), n, ma, A, lda, cnt, Bb, ldb, s->parts, (long)grid);
    else
      hipLaunchKernelGGL(bv_gram_kernel<false>, g, dim3(kBvBlock), 0, stream(), n, ma, A, lda, cnt, Bb, ldb, s->parts, (long)grid);
    PSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bv_gram_finish_kernel, dim3(ma * cnt), dim3(grid > kTailGroup ? kReduceBlock : 64), 0, stream(),
                       s->parts, grid, (long)grid, ma, G_dev + (size_t)b0 * ldg, ldg);
    PSP_LAUNCH_CHECK();
  }
  return PSP_OK;
}

int bv_resid(long n, int k, const double *AX, long ldax, const double *MX, long ldmx, const double *theta_dev,
             const int *slot_host, double *R, long ldr, double *nrm2_dev) {
  if (k <= 0) return PSP_OK;
  if (k > kResidMaxCols) return fail(PSP_EINVAL, "bv_resid: k = %d beyond %d", k, kResidMaxCols);
  if (n <= 0) {
    PSP_HIP(hipMemsetAsync(nrm2_dev, 0, sizeof(double) * (size_t)k, stream()));
    return PSP_OK;
  }
  BvSlots slots;
  for (int c = 0; c < kResidMaxCols; ++c) slots.s[c] = c < k ? slot_host[c] : -1;
  const int grid = bv_grid(n);
  BvScratch *s;
  PSP_TRY(bv_scratch((size_t)k * grid, &s));
  // the form bv_tdot takes for one stored column with itself; the wide accesses need the other two blocks aligned as well
  const bool pair = (n % 2 == 0) && (ldr % 2 == 0) && aligned16(R);
  const bool vload = pair && (ldax % 2 == 0) && (ldmx % 2 == 0) && aligned16(AX) && aligned16(MX);
#define L(P, V)                                                                                                       \
  hipLaunchKernelGGL((bv_resid_kernel<P, V>), dim3(grid, k), dim3(kBvBlock), 0, stream(), n, AX, ldax, MX, ldmx, theta_dev, \
                     slots, R, ldr, s->parts, (long)grid)
  if (vload) L(true, true);
  else if (pair) L(true, false);
  else L(false, false);
#undef L
  PSP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bv_tdot_finish_kernel, dim3(k), dim3(grid > kTailGroup ? kReduceBlock : 64), 0, stream(), s->parts,
                     grid, (long)grid, nrm2_dev);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int bv_tdot(long n, int m, const double *V, long ld, const double *x, double *h_dev) {
  if (m <= 0) return PSP_OK;
  if (n <= 0) {
    PSP_HIP(hipMemsetAsync(h_dev, 0, sizeof(double) * (size_t)m, stream()));
    return PSP_OK;
  }
  const int grid = bv_grid(n);
  BvScratch *s;
  PSP_TRY(bv_scratch((size_t)m * grid, &s));
  const int groups = (m + kTdotCols - 1) / kTdotCols;
  const bool vec = (n % 2 == 0) && (ld % 2 == 0) && aligned16(V) && aligned16(x);
  if (vec)
    hipLaunchKernelGGL(bv_tdot_kernel<true>, dim3(grid, groups), dim3(kBvBlock), 0, stream(), n, m, V, ld, x, s->parts,
                       (long)grid);
  else
    hipLaunchKernelGGL(bv_tdot_kernel<false>, dim3(grid, groups), dim3(kBvBlock), 0, stream(), n, m, V, ld, x, s->parts,
                       (long)grid);
  PSP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bv_tdot_finish_kernel, dim3(m), dim3(grid > kTailGroup ? kReduceBlock : 64), 0, stream(), s->parts,
                     grid, (long)grid, h_dev);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int bv_gemv(long n, int m, const double *V, long ld, const double *h_dev, double alpha, double beta, double *y) {
  if (n <= 0) return PSP_OK;
  if (m < 0) m = 0;
  PSP_TRY(ensure_device());
  const int grid = bv_grid(n);
  const bool vec = (n % 2 == 0) && (m == 0 || ((ld % 2 == 0) && aligned16(V))) && aligned16(y);
#define L(VEC, B0)                                                                                                  \
  hipLaunchKernelGGL((bv_gemv_kernel<VEC, B0>), dim3(grid), dim3(kBvBlock), 0, stream(), n, m, V, ld, h_dev, alpha, \
                     beta, y)
  if (beta == 0.0) {
    if (vec) L(true, true);
    else L(false, true);
  } else {
    if (vec) L(true, false);
    else L(false, false);
  }
#undef L
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int bv_rotate(long n, int j, double *V, long ld, const double *U_host, int ldu, int u0, int jn, int dst0) {
  if (j < 0 || j > kRotMaxJ) return fail(PSP_EINVAL, "bv_rotate: j = %d outside 0 .. %d", j, kRotMaxJ);
  if (jn < 0 || u0 < 0 || dst0 < 0 || u0 + jn > j || dst0 + jn > j || ldu < j)
    return fail(PSP_EINVAL, "bv_rotate: columns u0 = %d, jn = %d, dst0 = %d do not fit j = %d (ldu %d)", u0, jn, dst0, j, ldu);
  if (n <= 0 || jn == 0 || j == 0) return PSP_OK;
  BvScratch *s;
  PSP_TRY(bv_scratch(0, &s));
  if (!s->U) PSP_HIP(hipMalloc((void **)&s->U, sizeof(double) * kRotMaxJ * kRotMaxJ));
  // the used columns of U, compact; the copy is in stream order behind the previous rotate that read the buffer.  U_host is
  // borrowed for the call only (the eigensolver overwrites it right afterwards) and is pageable memory, whose asynchronous
  // copy may read it after the call has returned: wait for the copy -- the kernel behind it still runs asynchronously
  PSP_HIP(hipMemcpy2DAsync(s->U, sizeof(double) * j, U_host + (size_t)u0 * ldu, sizeof(double) * ldu, sizeof(double) * j, jn,
                           hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  const long grid = (n + kRotRows - 1) / kRotRows;
  hipLaunchKernelGGL(bv_rotate_kernel, dim3((unsigned)grid), dim3(kRotRows), sizeof(double) * kRotRows * (size_t)j, stream(),
                     n, j, V, ld, s->U, jn, dst0);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

// the rotate once more with the coefficients the calling thread's last bv_rotate uploaded (same j, same columns of U):
// the images A V and M V of a block follow it without another copy of U
int bv_rotate_again(long n, int j, double *V, long ld, int jn, int dst0) {
  if (j < 0 || j > kRotMaxJ || jn < 0 || dst0 < 0 || dst0 + jn > j)
    return fail(PSP_EINVAL, "bv_rotate_again: columns jn = %d, dst0 = %d do not fit j = %d", jn, dst0, j);
  if (n <= 0 || jn == 0 || j == 0) return PSP_OK;
  BvScratch *s;
  PSP_TRY(bv_scratch(0, &s));
  if (!s->U) return fail(PSP_EINVAL, "bv_rotate_again: no coefficients uploaded on this thread");
  const long grid = (n + kRotRows - 1) / kRotRows;
  hipLaunchKernelGGL(bv_rotate_kernel, dim3((unsigned)grid), dim3(kRotRows), sizeof(double) * kRotRows * (size_t)j, stream(),
                     n, j, V, ld, s->U, jn, dst0);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

}  // namespace psp

using namespace psp;

static int bv_check(const char *what, int n, int m, const void *V, int64_t ld, const void *a, const void *b) {
  if (n < 0 || m < 0) return fail(PSP_EINVAL, "%s: negative size", what);
  if (m > 0 && (!V || ld < n)) return fail(PSP_EINVAL, "%s: V is NULL or ld < n", what);
  if ((n > 0 && !a) || (m > 0 && !b)) return fail(PSP_EINVAL, "%s: NULL argument", what);
  if (cpu_mode()) return fail(PSP_ENODEV, "%s: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)", what);
  return ensure_device();
}

extern "C" {

int psp_bv_tdot(int n, int m, const double *V_dev, int64_t ld, const double *x_dev, double *h_dev) {
  PSP_TRY(bv_check("psp_bv_tdot", n, m, V_dev, ld, x_dev, h_dev));
  return bv_tdot(n, m, V_dev, (long)ld, x_dev, h_dev);
}

int psp_bv_gemv(int n, int m, const double *V_dev, int64_t ld, const double *h_dev, double alpha, double beta,
                double *y_dev) {
  PSP_TRY(bv_check("psp_bv_gemv", n, m, V_dev, ld, y_dev, h_dev));
  return bv_gemv(n, m, V_dev, (long)ld, h_dev, alpha, beta, y_dev);
}

int psp_bv_rotate(int n, int j, double *V_dev, int64_t ld, const double *U_host, int ldu, int u0, int jn, int dst0) {
  PSP_TRY(bv_check("psp_bv_rotate", n, j, V_dev, ld, V_dev, U_host));
  return bv_rotate(n, j, V_dev, (long)ld, U_host, ldu, u0, jn, dst0);
}

int psp_bv_gram(int n, int ma, const double *A_dev, int64_t lda, int mb, const double *B_dev, int64_t ldb, double *G_dev,
                int64_t ldg) {
  if (n < 0 || ma < 0 || mb < 0) return fail(PSP_EINVAL, "psp_bv_gram: negative size");
  if (ma > 0 && mb > 0 && (!A_dev || !B_dev || !G_dev || lda < n || ldb < n || ldg < ma))
    return fail(PSP_EINVAL, "psp_bv_gram: NULL argument or a leading dimension below the column length");
  if (cpu_mode()) return fail(PSP_ENODEV, "psp_bv_gram: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  PSP_TRY(ensure_device());
  return bv_gram(n, ma, A_dev, (long)lda, mb, B_dev, (long)ldb, G_dev, (long)ldg);
}

int psp_bv_resid(int n, int k, const double *AX_dev, int64_t ldax, const double *MX_dev, int64_t ldmx, const double *theta_dev,
                 const int *slot_host, double *R_dev, int64_t ldr, double *nrm2_dev) {
  if (n < 0 || k < 0 || k > kResidMaxCols) return fail(PSP_EINVAL, "psp_bv_resid: n negative or k outside 0 .. %d", kResidMaxCols);
  if (k > 0 && (!AX_dev || !MX_dev || !theta_dev || !slot_host || !nrm2_dev || ldax < n || ldmx < n))
    return fail(PSP_EINVAL, "psp_bv_resid: NULL argument or a leading dimension below n");
  bool stores = false;
  for (int c = 0; c < k; ++c) {
    if (slot_host[c] >= k) return fail(PSP_EINVAL, "psp_bv_resid: slot[%d] = %d beyond the %d columns of R", c, slot_host[c], k);
    for (int e = 0; e < c; ++e)
      if (slot_host[c] >= 0 && slot_host[e] == slot_host[c]) return fail(PSP_EINVAL, "psp_bv_resid: slot %d given twice", slot_host[c]);
    stores = stores || slot_host[c] >= 0;
  }
  if (stores && (!R_dev || ldr < n)) return fail(PSP_EINVAL, "psp_bv_resid: R is NULL or ldr < n");
  if (cpu_mode()) return fail(PSP_ENODEV, "psp_bv_resid: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  PSP_TRY(ensure_device());
  return bv_resid(n, k, AX_dev, (long)ldax, MX_dev, (long)ldmx, theta_dev, slot_host, R_dev, (long)ldr, nrm2_dev);
}

}  // extern "C"
