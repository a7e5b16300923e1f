// psp_mg.hip -- precon.multigrid(A, grid, omega, steps): a matrix-free geometric V-cycle for the constant-coefficient
// grid operators A = sum_a c_a T_a + s I (T_a = [-1 2 -1] along axis a, nothing stored across line ends; row
// k = i0 + n0 i1 + n0 n1 i2, the ordering of tools/poisson.py).  No reference analogue: the reference's preconditioners
// are jacobi and ssor (preconmodule.c).
//
// The cycle (DESIGN.md section 9c is the normative text):
//   * level l -> l + 1 coarsens every axis with n_a >= 4: n_a' = n_a / 2, coarse point j at fine index 2 j + 1,
//     c_a' = c_a / 4 on the coarsened axes; s' = s; the level's diagonal is d = 2 sum_{n_a > 1} c_a + s;
//   * P = (x)_a P_a with P_a[2j+1, j] = 1, P_a[2j, j] = P_a[2j+2, j] = 1/2 where in range; R = P' / 2^(coarsened axes);
//   * V(l, b): x = 0; `steps` sweeps x <- x + (omega / d)(b - A_l x); b_c = R (b - A_l x); x <- x + P V(l + 1, b_c);
//     `steps` sweeps; the coarsest level (no axis >= 4: at most 27 points) is a dense product with the inverse formed
//     on the host at creation.
// Nothing of a level is stored but its vectors: c_a, s and the dimensions are kernel arguments, Dirichlet ends are
// handled by omission.  Every sum has one fixed order and there are no atomics: the same bits from run to run.
//
// Kernels: mg_scale / mg_smooth (one out-of-place sweep; the first two sweeps from x = 0 in one pass over b),
// mg_restrict (a workgroup owns a tile of coarse points, forms the fine residuals of the tile plus halo in LDS and
// writes only b_c), mg_prolong (x += P e), mg_tail (the largest level of at most kTailT points and everything below
// it, down and up, dense solve included, in ONE launch of one workgroup with the vectors in LDS).
//
// galerkin = True (psp_mg_create_*_galerkin) is the same cycle for any symmetric 3- / 5- / 7-point
// operator on the grid, with stored level operators A_{l+1} = R A_l P.  The cycle kernels exist once: each is written
// against a level-operator policy Op that supplies the level's geometry, (A_l x)[i], omega / diagonal and the index
// split -- MfOp here (c_a and d are kernel arguments), GOp / GTailOp in psp_mg_galerkin.h (stored arrays), which this
// file includes and which holds what only the stored mode has; its creation is below, next to the matrix-free one.
//
// Blocks of k vectors (psp_mg_precon_block): block forms of the five cycle kernels, one thread per
// point and up to KC columns, the row's coefficients loaded once per point (Op::load_row / ax_row); the same schedule, the
// same launches whatever k is, column c with the bits of the single cycle on column c.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "psp_internal.h"

using namespace psp;

namespace {

constexpr int kTailThreads = 1024;
constexpr int kTailPts = 2;                        // points of a level per thread of the tail's workgroup
constexpr int kTailT = kTailThreads * kTailPts;    // largest level the tail takes
constexpr int kTailMaxLev = 12;                    // 2048 -> 1024 -> ... -> 4 -> 2 in 1-D is 11 levels
constexpr int kCoarsestMax = 27;                   // no axis >= 4: at most 3^3 points
constexpr int kMaxLevels = 32;                     // n < 2^31 and every level at least halves
// LDS of the tail (doubles): x and b of every level (level sizes at least halve: their sum stays below 2 kTailT), one
// level-sized scratch for the residual, the dense inverse
constexpr int kTailLds = 5 * kTailT + kCoarsestMax * kCoarsestMax;
// mg_restrict: 256 coarse points per workgroup; the fine residuals of the tile plus halo (2 t + 1 per coarsened axis)
constexpr int kResThreads = 256;
constexpr int kResLds = 33 * 9 * 9;  // the 3-D tile 16 x 4 x 4; 2-D 32 x 8 -> 65 x 17, 1-D 256 -> 513 are smaller

struct MgLevelArg {
  int n[3];     // dimensions (1 on the axes the grid does not have)
  int co[3];    // 1: the axis is coarsened towards the next level
  int nc[3];    // dimensions of the next level
  double c[3];  // 0 on axes of length 1
  double d;     // 2 sum c + s
  double w;     // omega / d
  double rs;    // 1 / 2^(coarsened axes)
};

template <class LevelT>  // what the mode keeps of a level: MgLevelArg, or psp_mg_galerkin.h's GLevel
struct TailArg {
  int nlev;
  int steps;
  int off[kTailMaxLev];  // offset of the level's x (and, kTailT * 2 further, b) in the tail's LDS
  LevelT lev[kTailMaxLev];
};

// (A_l x)[i]: the diagonal first, then axis by axis the lower and the upper neighbour -- one fixed order everywhere
template <class X>
__device__ __forceinline__ double mg_ax(const MgLevelArg &L, const X &x, long i, int i0, int i1, int i2) {
  double acc = L.d * x(i);
  if (L.n[0] > 1) {
    if (i0 > 0) acc -= L.c[0] * x(i - 1);
    if (i0 < L.n[0] - 1) acc -= L.c[0] * x(i + 1);
  }
  if (L.n[1] > 1) {
    const long s1 = L.n[0];
    if (i1 > 0) acc -= L.c[1] * x(i - s1);
    if (i1 < L.n[1] - 1) acc -= L.c[1] * x(i + s1);
  }
  if (L.n[2] > 1) {
    const long s2 = (long)L.n[0] * L.n[1];
    if (i2 > 0) acc -= L.c[2] * x(i - s2);
    if (i2 < L.n[2] - 1) acc -= L.c[2] * x(i + s2);
  }
  return acc;
}

// ND: axes the level's index is split into
template <int ND = 3>
__device__ __forceinline__ void mg_split(const MgLevelArg &L, long i, int &i0, int &i1, int &i2) {
  i0 = (int)i, i1 = 0, i2 = 0;
  if constexpr (ND == 2) {
    i0 = (int)(i % L.n[0]);
    i1 = (int)(i / L.n[0]);
  } else if constexpr (ND == 3) {
    i0 = (int)(i % L.n[0]);
    const long q = i / L.n[0];
    i1 = (int)(q % L.n[1]);
    i2 = (int)(q / L.n[1]);
  }
}

// The level-operator policy of the matrix-free mode: the level is its MgLevelArg, held by value (a kernel argument, or
// the tail's copy of its table entry in registers).  With ND < 3 the dead axes are set to length 1 so that their terms
// of mg_ax compile away; MfOp<3> takes any level as it is (the restriction and the tail, whose shapes are run-time).
template <int ND>
struct MfOp {
  using Level = MgLevelArg;
  MgLevelArg L;
  __device__ __forceinline__ explicit MfOp(const MgLevelArg &a) : L(a) {
    if constexpr (ND < 3) L.n[2] = 1;
    if constexpr (ND < 2) L.n[1] = 1;
  }
  __device__ __forceinline__ const MgLevelArg &geo() const { return L; }
  template <class X>
  __device__ __forceinline__ double ax(const X &x, long i, int i0, int i1, int i2) const {
    return mg_ax(L, x, i, i0, i1, i2);
  }
  __device__ __forceinline__ double w(long) const { return L.w; }
  __device__ __forceinline__ void split(long i, int &i0, int &i1, int &i2) const { mg_split<ND>(L, i, i0, i1, i2); }
  // the block kernels' pair (GOp in psp_mg_galerkin.h has the real one): this mode's row is kernel arguments, nothing is
  // loaded; x(j, w_j) is the column's value at j
  struct Row {
    double w;
  };
  template <bool WN>
  __device__ __forceinline__ Row load_row(long, int, int, int) const {
    return Row{L.w};
  }
  template <class X>
  __device__ __forceinline__ double ax_row(const Row &r, const X &x, long i, int i0, int i1, int i2) const {
    auto X1 = [&](long j) { return x(j, r.w); };
    return mg_ax(L, X1, i, i0, i1, i2);
  }
};
// omega / d as mg_scale_kernel takes it
struct MfW {
  double w;
  __device__ __forceinline__ double operator()(long) const { return w; }
};
__host__ __device__ inline const MgLevelArg &level_geo(const MgLevelArg &a) { return a; }

// (R r)[j] for the coarse point (j0, j1, j2); r is indexed through `at(l0, l1, l2)` with fine coordinates, which returns 0
// outside the grid.  Weights 1/2, 1, 1/2 along a coarsened axis at fine 2j, 2j+1, 2j+2; axis 2 outermost, ascending.
template <class AT>
__device__ __forceinline__ double mg_restrict_point(const MgLevelArg &L, const AT &at, int j0, int j1, int j2) {
  const int b0 = L.co[0] ? 2 * j0 : j0, m0 = L.co[0] ? 3 : 1;
  const int b1 = L.co[1] ? 2 * j1 : j1, m1 = L.co[1] ? 3 : 1;
  const int b2 = L.co[2] ? 2 * j2 : j2, m2 = L.co[2] ? 3 : 1;
  double sum = 0.0;
  for (int k2 = 0; k2 < m2; ++k2) {
    const double w2 = (L.co[2] && k2 != 1) ? 0.5 : 1.0;
    for (int k1 = 0; k1 < m1; ++k1) {
      const double w1 = (L.co[1] && k1 != 1) ? 0.5 * w2 : w2;
      for (int k0 = 0; k0 < m0; ++k0) {
        const double w0 = (L.co[0] && k0 != 1) ? 0.5 * w1 : w1;
        sum += w0 * at(b0 + k0, b1 + k1, b2 + k2);
      }
    }
  }
  return sum * L.rs;
}

// (P e)[i] for the fine point (i0, i1, i2); e is the next level's vector.  Along a coarsened axis an odd index takes
// coarse (i - 1) / 2 whole, an even one half of coarse i / 2 - 1 and half of i / 2 where they exist; lower before upper,
// axis 2 outermost.
struct MgAxisSrc {
  int ja, jb, cnt;  // the coarse indices a fine index takes from (jb only when cnt == 2)
  double wt;
};
__device__ __forceinline__ MgAxisSrc mg_axis_src(int co, int g, int nc) {
  MgAxisSrc s;
  s.jb = 0;
  if (!co) {
    s.ja = g, s.cnt = 1, s.wt = 1.0;
  } else if (g & 1) {
    s.ja = (g - 1) >> 1, s.cnt = 1, s.wt = 1.0;
  } else {
    const int lo = (g >> 1) - 1, hi = g >> 1;  // at least one exists: nc >= 2 on a coarsened axis
    s.wt = 0.5;
    if (lo >= 0 && hi < nc) {
      s.ja = lo, s.jb = hi, s.cnt = 2;
    } else {
      s.ja = lo >= 0 ? lo : hi, s.cnt = 1;
    }
  }
  return s;
}
template <class E>
__device__ __forceinline__ double mg_prolong_point(const MgLevelArg &L, const E &e, int i0, int i1, int i2) {
  const MgAxisSrc a0 = mg_axis_src(L.co[0], i0, L.nc[0]), a1 = mg_axis_src(L.co[1], i1, L.nc[1]),
                  a2 = mg_axis_src(L.co[2], i2, L.nc[2]);
  const double w = a0.wt * a1.wt * a2.wt;  // powers of two: exact
  double sum = 0.0;
  for (int k2 = 0; k2 < a2.cnt; ++k2) {
    const long j2 = k2 ? a2.jb : a2.ja;
    for (int k1 = 0; k1 < a1.cnt; ++k1) {
      const long j1 = k1 ? a1.jb : a1.ja;
      for (int k0 = 0; k0 < a0.cnt; ++k0) {
        const long j0 = k0 ? a0.jb : a0.ja;
        sum += w * e(j0 + (long)L.nc[0] * (j1 + (long)L.nc[1] * j2));
      }
    }
  }
  return sum;
}

// ------------------------------------------------------------------ the launch-per-step kernels of the large levels

// the first sweep from x = 0: x = 0 + (omega / d)(b - 0) = (omega / d) b; W: MfW (a scalar) or GW (an array)
template <class W>
__global__ __launch_bounds__(256) void mg_scale_kernel(long N, W w, const double *__restrict__ b, double *__restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < N) x[i] = w(i) * b[i];
}

// one sweep, out of place: xout = xin + (omega / d)(b - A xin); reads xin and b (and, with a stored stencil, w and every
// coefficient array) once, writes xout once; the neighbours (of xin, and the neighbours' rows of the lower arrays: the
// upper couplings) come from the caches.  FROMB: xin is the first sweep's (omega / d) b, formed on the fly -- sweeps one
// and two of a cycle in one pass.
template <class Op, bool FROMB>
__global__ __launch_bounds__(256) void mg_smooth_kernel(typename Op::Level A, long N, const double *__restrict__ xin,
                                                        const double *__restrict__ b, double *__restrict__ xout) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const Op op(A);
  int i0, i1, i2;
  op.split(i, i0, i1, i2);
  auto X = [&](long k) { return FROMB ? op.w(k) * b[k] : xin[k]; };
  const double ax = op.ax(X, i, i0, i1, i2);
  xout[i] = X(i) + op.w(i) * (b[i] - ax);
}

// b_c = R (b - A x): blockIdx.x = the tile of coarse points (t[0] x t[1] x t[2] = 256 of them), `r` = the fine residuals
// the tile's restriction reads; a fine point outside the grid counts as 0.  The fine residual never reaches memory.
template <class Op>
__global__ __launch_bounds__(kResThreads) void mg_restrict_kernel(typename Op::Level A, int t0, int t1, int t2, int g0n,
                                                                  int g1n, const double *__restrict__ x,
                                                                  const double *__restrict__ b,
                                                                  double *__restrict__ bc) {
  __shared__ double r[kResLds];
  const Op op(A);
  const MgLevelArg &L = op.geo();
  // the tile's three indices ride in blockIdx.x (g0n x g1n x g2n tiles, axis 0 fastest): a long second or third axis
  // would not fit gridDim.y / gridDim.z
  const unsigned bq = blockIdx.x / (unsigned)g0n;
  const int J0 = (int)(blockIdx.x % (unsigned)g0n) * t0, J1 = (int)(bq % (unsigned)g1n) * t1, J2 = (int)(bq / (unsigned)g1n) * t2;
  const int f0 = L.co[0] ? 2 * J0 : J0, F0 = L.co[0] ? 2 * t0 + 1 : t0;
  const int f1 = L.co[1] ? 2 * J1 : J1, F1 = L.co[1] ? 2 * t1 + 1 : t1;
  const int f2 = L.co[2] ? 2 * J2 : J2, F2 = L.co[2] ? 2 * t2 + 1 : t2;
  const int total = F0 * F1 * F2;  // <= kResLds (mg_tile)
  auto X = [&](long k) { return x[k]; };
  for (int t = threadIdx.x; t < total; t += kResThreads) {
    const int l0 = t % F0, q = t / F0, l1 = q % F1, l2 = q / F1;
    const int g0 = f0 + l0, g1 = f1 + l1, g2 = f2 + l2;
    double v = 0.0;
    if (g0 < L.n[0] && g1 < L.n[1] && g2 < L.n[2]) {
      const long i = g0 + (long)L.n[0] * (g1 + (long)L.n[1] * g2);
      v = b[i] - op.ax(X, i, g0, g1, g2);
    }
    r[t] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < t0 * t1 * t2) {
    const int j0 = t % t0, q = t / t0, j1 = q % t1, j2 = q / t1;
    if (J0 + j0 < L.nc[0] && J1 + j1 < L.nc[1] && J2 + j2 < L.nc[2]) {
      // the tile's fine region starts at the fine image of its first coarse point: local fine coordinates
      auto at = [&](int a0, int a1, int a2) { return r[a0 + F0 * (a1 + F1 * a2)]; };
      const double v = mg_restrict_point(L, at, j0, j1, j2);
      bc[(J0 + j0) + (long)L.nc[0] * ((J1 + j1) + (long)L.nc[1] * (J2 + j2))] = v;
    }
  }
}

// x += P e: reads x and e, writes x
__global__ __launch_bounds__(256) void mg_prolong_kernel(MgLevelArg L, long N, const double *__restrict__ e,
                                                         double *__restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int i0, i1, i2;
  mg_split(L, i, i0, i1, i2);
  auto E = [&](long k) { return e[k]; };
  x[i] = x[i] + mg_prolong_point(L, E, i0, i1, i2);
}

// ------------------------------------------------------------------ the block forms: k columns at once (section 9e)
// Column c of a vector block starts at base + c * ld.  A thread owns one point and up to KC columns (blockIdx.y = the
// group of KC columns): the index split, omega / diagonal and the row's coefficients are formed or loaded once
// (Op::load_row), then each column gets the single kernel's arithmetic in the single kernel's order (Op::ax_row).
// frozen != nullptr: a column with frozen[c] != 0 is skipped -- nothing of it is read or written; the branch is uniform
// across the workgroup.

// live columns of the group that starts at c0, as a bit mask
template <int KC>
__device__ __forceinline__ unsigned mg_live(int c0, int k, const int *__restrict__ frozen) {
  unsigned m = 0u;
#pragma unroll
  for (int c = 0; c < KC; ++c)
    if (c0 + c < k && !(frozen && frozen[c0 + c])) m |= 1u << c;
  return m;
}

template <class W, int KC>
__global__ __launch_bounds__(256) void mg_scale_block_kernel(long N, W w, int k, const double *__restrict__ b, long ldb,
                                                             double *__restrict__ x, long ldx,
                                                             const int *__restrict__ frozen) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * KC;
  const unsigned live = mg_live<KC>(c0, k, frozen);
  if (i >= N || !live) return;
  const double wi = w(i);
#pragma unroll
  for (int c = 0; c < KC; ++c)
    if ((live >> c) & 1u) x[(size_t)(c0 + c) * ldx + i] = wi * b[(size_t)(c0 + c) * ldb + i];
}

template <class Op, bool FROMB, int KC>
__global__ __launch_bounds__(256) void mg_smooth_block_kernel(typename Op::Level A, long N, int k,
                                                              const double *__restrict__ xin, long ldi,
                                                              const double *__restrict__ b, long ldb,
                                                              double *__restrict__ xout, long ldo,
                                                              const int *__restrict__ frozen) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * KC;
  const unsigned live = mg_live<KC>(c0, k, frozen);
  if (i >= N || !live) return;
  const Op op(A);
  int i0, i1, i2;
  op.split(i, i0, i1, i2);
  const auto row = op.template load_row<FROMB>(i, i0, i1, i2);
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    if (!((live >> c) & 1u)) continue;
    const double *__restrict__ bc = b + (size_t)(c0 + c) * ldb;
    const double *__restrict__ xc = FROMB ? bc : xin + (size_t)(c0 + c) * ldi;
    auto X = [&](long j, double wj) { return FROMB ? wj * bc[j] : xc[j]; };
    const double ax = op.ax_row(row, X, i, i0, i1, i2);
    xout[(size_t)(c0 + c) * ldo + i] = X(i, row.w) + row.w * (bc[i] - ax);
  }
}

// b_c = R (b - A x) for KC columns: points outer, columns inner -- a fine point's row is loaded once and applied to every
// column of the group, whose residual tiles lie side by side in LDS.  KC = 1 with the columns in gridDim.y is the other
// form (one tile, reused by nobody: every column is a workgroup of its own).
template <class Op, int KC>
__global__ __launch_bounds__(kResThreads) void mg_restrict_block_kernel(typename Op::Level A, int t0, int t1, int t2,
                                                                        int g0n, int g1n, int k,
                                                                        const double *__restrict__ x, long ldx,
                                                                        const double *__restrict__ b, long ldb,
                                                                        double *__restrict__ bc, long ldc,
                                                                        const int *__restrict__ frozen) {
  __shared__ double r[KC][kResLds];
  const int c0 = blockIdx.y * KC;
  const unsigned live = mg_live<KC>(c0, k, frozen);
  if (!live) return;  // uniform: before any barrier
  const Op op(A);
  const MgLevelArg &L = op.geo();
  const unsigned bq = blockIdx.x / (unsigned)g0n;
  const int J0 = (int)(blockIdx.x % (unsigned)g0n) * t0, J1 = (int)(bq % (unsigned)g1n) * t1, J2 = (int)(bq / (unsigned)g1n) * t2;
  const int f0 = L.co[0] ? 2 * J0 : J0, F0 = L.co[0] ? 2 * t0 + 1 : t0;
  const int f1 = L.co[1] ? 2 * J1 : J1, F1 = L.co[1] ? 2 * t1 + 1 : t1;
  const int f2 = L.co[2] ? 2 * J2 : J2, F2 = L.co[2] ? 2 * t2 + 1 : t2;
  const int total = F0 * F1 * F2;  // <= kResLds (mg_tile)
  for (int t = threadIdx.x; t < total; t += kResThreads) {
    const int l0 = t % F0, q = t / F0, l1 = q % F1, l2 = q / F1;
    const int g0 = f0 + l0, g1 = f1 + l1, g2 = f2 + l2;
    if (g0 < L.n[0] && g1 < L.n[1] && g2 < L.n[2]) {
      const long i = g0 + (long)L.n[0] * (g1 + (long)L.n[1] * g2);
      const auto row = op.template load_row<false>(i, g0, g1, g2);
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        if (!((live >> c) & 1u)) continue;
        const double *__restrict__ xc = x + (size_t)(c0 + c) * ldx;
        auto X = [&](long j, double) { return xc[j]; };
        r[c][t] = b[(size_t)(c0 + c) * ldb + i] - op.ax_row(row, X, i, g0, g1, g2);
      }
    } else {
#pragma unroll
      for (int c = 0; c < KC; ++c) r[c][t] = 0.0;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < t0 * t1 * t2) {
    const int j0 = t % t0, q = t / t0, j1 = q % t1, j2 = q / t1;
    if (J0 + j0 < L.nc[0] && J1 + j1 < L.nc[1] && J2 + j2 < L.nc[2]) {
      const long jc = (J0 + j0) + (long)L.nc[0] * ((J1 + j1) + (long)L.nc[1] * (J2 + j2));
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        if (!((live >> c) & 1u)) continue;
        const double *rc = r[c];
        auto at = [&](int a0, int a1, int a2) { return rc[a0 + F0 * (a1 + F1 * a2)]; };
        bc[(size_t)(c0 + c) * ldc + jc] = mg_restrict_point(L, at, j0, j1, j2);
      }
    }
  }
}

// x += P e: one index split per point, then the columns
template <int KC>
__global__ __launch_bounds__(256) void mg_prolong_block_kernel(MgLevelArg L, long N, int k, const double *__restrict__ e,
                                                               long lde, double *__restrict__ x, long ldx,
                                                               const int *__restrict__ frozen) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * KC;
  const unsigned live = mg_live<KC>(c0, k, frozen);
  if (i >= N || !live) return;
  int i0, i1, i2;
  mg_split(L, i, i0, i1, i2);
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    if (!((live >> c) & 1u)) continue;
    const double *__restrict__ ec = e + (size_t)(c0 + c) * lde;
    double *__restrict__ xc = x + (size_t)(c0 + c) * ldx;
    auto E = [&](long j) { return ec[j]; };
    xc[i] = xc[i] + mg_prolong_point(L, E, i0, i1, i2);
  }
}

// ------------------------------------------------------------------ the tail: one workgroup, vectors in LDS

// one sweep of a level in LDS: every thread forms its points' new values, then all are written
template <class Op>
__device__ __forceinline__ void tail_sweep(const Op &op, int N, double *xs, const double *bs) {
  auto X = [&](long k) { return xs[k]; };
  double xn[kTailPts];
#pragma unroll
  for (int p = 0; p < kTailPts; ++p) {
    const int i = threadIdx.x + p * kTailThreads;
    xn[p] = 0.0;
    if (i < N) {
      int i0, i1, i2;
      op.split(i, i0, i1, i2);
      xn[p] = xs[i] + op.w(i) * (bs[i] - op.ax(X, i, i0, i1, i2));
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < kTailPts; ++p) {
    const int i = threadIdx.x + p * kTailThreads;
    if (i < N) xs[i] = xn[p];
  }
  __syncthreads();
}

// Op: MfOp<3> (each level's MgLevelArg copied into registers) or GTailOp (the level's GLevel stays in global memory, and
// so do its coefficient arrays: 14 kTailT doubles for the top tail level alone do not fit LDS)
template <class Op>
__device__ __forceinline__ void mg_tail_body(const TailArg<typename Op::Level> *__restrict__ T,
                                             const double *__restrict__ minv, const double *__restrict__ bin,
                                             double *__restrict__ xout) {
  __shared__ double sh[kTailLds];
  double *const scr = sh + 4 * kTailT;
  double *const mi = sh + 5 * kTailT;
  const int nl = T->nlev, steps = T->steps, tid = threadIdx.x;
  {
    const MgLevelArg &L = level_geo(T->lev[0]);
    const int N = L.n[0] * L.n[1] * L.n[2];
    double *bs = sh + 2 * kTailT + T->off[0];
    for (int i = tid; i < N; i += kTailThreads) bs[i] = bin[i];
    const MgLevelArg &C = level_geo(T->lev[nl - 1]);
    const int nc = C.n[0] * C.n[1] * C.n[2];
    for (int i = tid; i < nc * nc; i += kTailThreads) mi[i] = minv[i];
  }
  __syncthreads();
  // down
  for (int l = 0; l < nl - 1; ++l) {
    const Op op(T->lev[l]);
    const MgLevelArg &L = op.geo();
    const int N = L.n[0] * L.n[1] * L.n[2], Nc = L.nc[0] * L.nc[1] * L.nc[2];
    double *xs = sh + T->off[l], *bs = sh + 2 * kTailT + T->off[l], *bn = sh + 2 * kTailT + T->off[l + 1];
    for (int i = tid; i < N; i += kTailThreads) xs[i] = op.w(i) * bs[i];
    __syncthreads();
    for (int k = 1; k < steps; ++k) tail_sweep(op, N, xs, bs);
    auto X = [&](long k) { return xs[k]; };
    for (int i = tid; i < N; i += kTailThreads) {
      int i0, i1, i2;
      op.split(i, i0, i1, i2);
      scr[i] = bs[i] - op.ax(X, i, i0, i1, i2);
    }
    __syncthreads();
    auto at = [&](int a0, int a1, int a2) {
      return (a0 < L.n[0] && a1 < L.n[1] && a2 < L.n[2]) ? scr[a0 + L.n[0] * (a1 + L.n[1] * a2)] : 0.0;
    };
    for (int j = tid; j < Nc; j += kTailThreads) {
      const int j0 = j % L.nc[0], q = j / L.nc[0], j1 = q % L.nc[1], j2 = q / L.nc[1];
      bn[j] = mg_restrict_point(L, at, j0, j1, j2);
    }
    __syncthreads();
  }
  // the coarsest level: x = A^-1 b with the inverse formed at creation
  {
    const MgLevelArg &C = level_geo(T->lev[nl - 1]);
    const int nc = C.n[0] * C.n[1] * C.n[2];
    double *xs = sh + T->off[nl - 1];
    const double *bs = sh + 2 * kTailT + T->off[nl - 1];
    if (tid < nc) {
      double s = 0.0;
      for (int j = 0; j < nc; ++j) s += mi[tid * nc + j] * bs[j];
      xs[tid] = s;
    }
    __syncthreads();
  }
  // up
  for (int l = nl - 2; l >= 0; --l) {
    const Op op(T->lev[l]);
    const MgLevelArg &L = op.geo();
    const int N = L.n[0] * L.n[1] * L.n[2];
    double *xs = sh + T->off[l];
    const double *bs = sh + 2 * kTailT + T->off[l], *en = sh + T->off[l + 1];
    auto E = [&](long k) { return en[k]; };
    for (int i = tid; i < N; i += kTailThreads) {
      int i0, i1, i2;
      mg_split(L, i, i0, i1, i2);
      xs[i] = xs[i] + mg_prolong_point(L, E, i0, i1, i2);
    }
    __syncthreads();
    for (int k = 0; k < steps; ++k) tail_sweep(op, N, xs, bs);
  }
  {
    const MgLevelArg &L = level_geo(T->lev[0]);
    const int N = L.n[0] * L.n[1] * L.n[2];
    const double *xs = sh + T->off[0];
    for (int i = tid; i < N; i += kTailThreads) xout[i] = xs[i];
  }
}

template <class Op>
__global__ __launch_bounds__(kTailThreads) void mg_tail_kernel(const TailArg<typename Op::Level> *__restrict__ T,
                                                               const double *__restrict__ minv,
                                                               const double *__restrict__ bin,
                                                               double *__restrict__ xout) {
  mg_tail_body<Op>(T, minv, bin, xout);
}

// the block form: workgroup c runs the tail on column c's pointers; a frozen column's workgroup returns at once
template <class Op>
__global__ __launch_bounds__(kTailThreads) void mg_tail_block_kernel(const TailArg<typename Op::Level> *__restrict__ T,
                                                                     const double *__restrict__ minv,
                                                                     const double *__restrict__ bin, long ldb,
                                                                     double *__restrict__ xout, long ldx,
                                                                     const int *__restrict__ frozen) {
  const int c = blockIdx.x;
  if (frozen && frozen[c]) return;
  mg_tail_body<Op>(T, minv, bin + (size_t)c * ldb, xout + (size_t)c * ldx);
}

// ------------------------------------------------------------------ the exact check at creation

// bit 0: the diagonal; bits 1 + 2a / 2 + 2a: the lower / upper neighbour along axis a
__device__ __forceinline__ unsigned mg_expected(int r, int n0, int n1, int n2) {
  const int i0 = r % n0, q = r / n0, i1 = q % n1, i2 = q / n1;
  unsigned m = 1u;
  if (i0 > 0) m |= 1u << 1;
  if (i0 < n0 - 1) m |= 1u << 2;
  if (i1 > 0) m |= 1u << 3;
  if (i1 < n1 - 1) m |= 1u << 4;
  if (i2 > 0) m |= 1u << 5;
  if (i2 < n2 - 1) m |= 1u << 6;
  return m;
}

struct MgStencil {
  int n[3];
  double c[3];
  double d0;
};

// every stored entry of every row is one the stencil has, with the stencil's value, and none is missing
__global__ __launch_bounds__(256) void mg_check_csr_kernel(int n, MgStencil S, const int *__restrict__ ind,
                                                           const int *__restrict__ col, const double *__restrict__ val,
                                                           int *__restrict__ bad) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const unsigned want = mg_expected(r, S.n[0], S.n[1], S.n[2]);
  const long st[3] = {1, S.n[0], (long)S.n[0] * S.n[1]};
  unsigned seen = 0;
  bool ok = true;
  for (int k = ind[r]; k < ind[r + 1]; ++k) {
    const long off = (long)col[k] - r;
    const double v = val[k];
    int bit = -1;
    double ev = 0.0;
    if (off == 0) {
      bit = 0;
      ev = S.d0;
    } else {
      for (int a = 0; a < 3; ++a)
        if (S.n[a] > 1 && (off == st[a] || off == -st[a])) {
          bit = 1 + 2 * a + (off > 0 ? 1 : 0);
          ev = -S.c[a];
        }
    }
    if (bit < 0 || !((want >> bit) & 1u) || ((seen >> bit) & 1u) || !(v == ev)) ok = false;
    if (bit >= 0) seen |= 1u << bit;
  }
  if (!ok || seen != want) *bad = 1;
}

// the same on the index-free layout: the values are constant per offset (checked on the host against the view's cval);
// bit o of mask[r] says that row r stores offset slot o, slotbit[o] is that offset's bit in mg_expected's numbering
struct MgSlots {
  int no;
  int bit[12];
};
__global__ __launch_bounds__(256) void mg_check_w4_kernel(int n, MgStencil S, MgSlots Q,
                                                          const unsigned short *__restrict__ mask,
                                                          int *__restrict__ bad) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const unsigned want = mg_expected(r, S.n[0], S.n[1], S.n[2]);
  const unsigned m = mask[r];
  unsigned seen = 0;
  for (int o = 0; o < Q.no; ++o)
    if ((m >> o) & 1u) seen |= 1u << Q.bit[o];
  if (seen != want || (m >> Q.no) != 0) *bad = 1;
}

}  // namespace

#include "psp_mg_galerkin.h"

// ====================================================================== the handle

struct psp_mg {
  int n = 0, ndim = 0, steps = 2;
  double omega = 0.8;
  struct Level {
    MgLevelArg a;
    long N = 0;
    double *x = nullptr, *b = nullptr, *t = nullptr;  // the level's vectors (levels in the tail have none)
  };
  std::vector<Level> lev;
  int tail_first = 0;  // first level of the tail launch
  int launches = 0;    // kernel launches of one application
  double *minv = nullptr;
  void *tail = nullptr;  // the mode's TailArg on the device
  // galerkin = True (psp_mg_galerkin.h): the stored level operators; `coef` owns each level's arrays in one allocation
  // (diagonal, omega / diagonal, the lower arrays)
  bool galerkin = false;
  std::vector<GLevel> glev;
  std::vector<double *> coef;
  // the level vectors of the block cycle (section 9e): per level what `lev` holds, for blk_cols columns of leading
  // dimension N, and a spare for the finest level; allocated by the first block call, grown on demand
  struct BlockLevel {
    double *x = nullptr, *b = nullptr, *t = nullptr;
  };
  std::vector<BlockLevel> blk;
  int blk_cols = 0;
  size_t blk_bytes = 0;
};

namespace {

int level_nd(const MgLevelArg &a) { return a.n[2] > 1 ? 3 : a.n[1] > 1 ? 2 : 1; }

// coarse points per workgroup of mg_restrict along each axis (256 in all): by the axes the level really has
void mg_tile(const MgLevelArg &a, int t[3]) {
  const int nd = level_nd(a);
  if (nd == 1) {
    t[0] = 256, t[1] = 1, t[2] = 1;
  } else if (nd == 2) {
    t[0] = 32, t[1] = 8, t[2] = 1;
  } else {
    t[0] = 16, t[1] = 4, t[2] = 4;
  }
}

// the inverse of the coarsest level's matrix (dense, <= 27 x 27, symmetric positive definite) by Gauss-Jordan
// elimination with partial pivoting
int dense_inverse(int m, std::vector<double> &M, std::vector<double> *out);

int coarsest_inverse(const MgLevelArg &a, std::vector<double> *out) {
  const int m = a.n[0] * a.n[1] * a.n[2];
  std::vector<double> M((size_t)m * m, 0.0);
  const int st[3] = {1, a.n[0], a.n[0] * a.n[1]};
  for (int r = 0; r < m; ++r) {
    const int g[3] = {r % a.n[0], (r / a.n[0]) % a.n[1], r / (a.n[0] * a.n[1])};
    M[(size_t)r * m + r] = a.d;
    for (int x = 0; x < 3; ++x) {
      if (a.n[x] <= 1) continue;
      if (g[x] > 0) M[(size_t)r * m + r - st[x]] = -a.c[x];
      if (g[x] < a.n[x] - 1) M[(size_t)r * m + r + st[x]] = -a.c[x];
    }
  }
  return dense_inverse(m, M, out);
}

// the inverse of the dense m x m matrix M (overwritten) by Gauss-Jordan elimination with partial pivoting
int dense_inverse(int m, std::vector<double> &M, std::vector<double> *out) {
  std::vector<double> I((size_t)m * m, 0.0);
  for (int r = 0; r < m; ++r) I[(size_t)r * m + r] = 1.0;
  for (int k = 0; k < m; ++k) {
    int p = k;
    for (int r = k + 1; r < m; ++r)
      if (std::fabs(M[(size_t)r * m + k]) > std::fabs(M[(size_t)p * m + k])) p = r;
    if (!(std::fabs(M[(size_t)p * m + k]) > 0.0)) return fail(PSP_ESINGULAR, "multigrid: the coarsest level is singular");
    if (p != k)
      for (int j = 0; j < m; ++j) {
        std::swap(M[(size_t)p * m + j], M[(size_t)k * m + j]);
        std::swap(I[(size_t)p * m + j], I[(size_t)k * m + j]);
      }
    const double piv = M[(size_t)k * m + k];
    for (int j = 0; j < m; ++j) {
      M[(size_t)k * m + j] /= piv;
      I[(size_t)k * m + j] /= piv;
    }
    for (int r = 0; r < m; ++r) {
      if (r == k) continue;
      const double f = M[(size_t)r * m + k];
      if (f == 0.0) continue;
      for (int j = 0; j < m; ++j) {
        M[(size_t)r * m + j] -= f * M[(size_t)k * m + j];
        I[(size_t)r * m + j] -= f * I[(size_t)k * m + j];
      }
    }
  }
  *out = I;
  return PSP_OK;
}

int read_flag(int *bad_dev, int *bad) {
  PSP_HIP(hipMemcpyAsync(bad, bad_dev, sizeof(int), hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

// one checking pass: launch(flag) with a zeroed device flag, then the flag read back into *bad
template <class Launch>
int run_check(int *bad, Launch &&launch) {
  int *bad_dev = nullptr;
  PSP_HIP(hipMalloc((void **)&bad_dev, sizeof(int)));
  hipError_t e = hipMemsetAsync(bad_dev, 0, sizeof(int), stream());
  if (e == hipSuccess) {
    launch(bad_dev);
    e = hipGetLastError();
  }
  const int rc = e == hipSuccess ? read_flag(bad_dev, bad) : fail(PSP_ENODEV, "multigrid: %s", hipGetErrorString(e));
  (void)hipFree(bad_dev);
  return rc;
}

// c_a, d0 of A and the exact check that A is that stencil on that grid -- from the CSR arrays, or, for a handle that only
// kept its index-free layout, from that layout's offsets, values and row masks
int read_stencil(const psp_csr *A, const int n[3], MgStencil *S) {
  const long st[3] = {1, n[0], (long)n[0] * n[1]};
  for (int a = 0; a < 3; ++a) {
    S->n[a] = n[a];
    S->c[a] = 0.0;
  }
  S->d0 = 0.0;
  bool have_d = false, have_c[3] = {false, false, false};
  int bad = 0;
  const char *why = "multigrid: the matrix is not a constant-coefficient [-1 2 -1] stencil on this grid";
  if (A->ind && A->col && A->val && !A->w4_only) {
    // row 0 has its upper neighbour along every axis: it names every coefficient
    int ind01[2];
    PSP_HIP(hipMemcpyAsync(ind01, A->ind, 2 * sizeof(int), hipMemcpyDeviceToHost, stream()));
    PSP_HIP(hipStreamSynchronize(stream()));
    const int len = ind01[1] - ind01[0];
    if (ind01[0] != 0 || len < 1 || len > 4) return fail(PSP_EINVAL, "%s (row 0 stores %d entries)", why, len);
    int col[4];
    double val[4];
    PSP_HIP(hipMemcpyAsync(col, A->col, len * sizeof(int), hipMemcpyDeviceToHost, stream()));
    PSP_HIP(hipMemcpyAsync(val, A->val, len * sizeof(double), hipMemcpyDeviceToHost, stream()));
    PSP_HIP(hipStreamSynchronize(stream()));
    for (int k = 0; k < len; ++k) {
      if (col[k] == 0) {
        S->d0 = val[k];
        have_d = true;
      }
      for (int a = 0; a < 3; ++a)
        if (n[a] > 1 && col[k] == st[a]) {
          S->c[a] = -val[k];
          have_c[a] = true;
        }
    }
  } else {
    W4View v;
    int avail = 0;
    PSP_TRY(csr_w4_view(A, &v, &avail));
    if (!avail || !v.constv || v.no > 7) return fail(PSP_EINVAL, "%s", why);
    MgSlots Q;
    Q.no = v.no;
    double lower[3] = {0.0, 0.0, 0.0};
    bool have_l[3] = {false, false, false};
    for (int o = 0; o < v.no; ++o) {
      int bit = -1;
      if (v.offs[o] == 0) {
        bit = 0;
        S->d0 = v.cval[o];
        have_d = true;
      }
      for (int a = 0; a < 3; ++a) {
        if (n[a] <= 1) continue;
        if (v.offs[o] == st[a]) {
          bit = 2 + 2 * a;
          S->c[a] = -v.cval[o];
          have_c[a] = true;
        } else if (v.offs[o] == -st[a]) {
          bit = 1 + 2 * a;
          lower[a] = -v.cval[o];
          have_l[a] = true;
        }
      }
      if (bit < 0) return fail(PSP_EINVAL, "%s (an entry at offset %d)", why, v.offs[o]);
      Q.bit[o] = bit;
    }
    for (int a = 0; a < 3; ++a)
      if (n[a] > 1 && (!have_c[a] || !have_l[a] || !(lower[a] == S->c[a]))) return fail(PSP_EINVAL, "%s", why);
    if (!have_d) return fail(PSP_EINVAL, "%s", why);
    PSP_TRY(run_check(&bad, [&](int *flag) {
      hipLaunchKernelGGL(mg_check_w4_kernel, dim3((A->nrows + 255) / 256), dim3(256), 0, stream(), A->nrows, *S, Q, v.mask, flag);
    }));
    if (bad) return fail(PSP_EINVAL, "%s", why);
    return PSP_OK;
  }
  if (!have_d) return fail(PSP_EINVAL, "%s (row 0 has no diagonal)", why);
  for (int a = 0; a < 3; ++a)
    if (n[a] > 1 && !have_c[a]) return fail(PSP_EINVAL, "%s (row 0 has no neighbour along axis %d)", why, a);
  PSP_TRY(run_check(&bad, [&](int *flag) {
    hipLaunchKernelGGL(mg_check_csr_kernel, dim3((A->nrows + 255) / 256), dim3(256), 0, stream(), A->nrows, *S, A->ind, A->col,
                       A->val, flag);
  }));
  if (bad) return fail(PSP_EINVAL, "%s", why);
  return PSP_OK;
}

// the argument checks both modes make before the first device call; n = the grid padded with ones
int mg_check_args(const psp_csr *A, int ndim, const int *grid, double omega, int steps, psp_mg **out, int n[3]) {
  if (!A || !grid || !out) return fail(PSP_EINVAL, "psp_mg_create: NULL argument");
  if (ndim < 1 || ndim > 3) return fail(PSP_EINVAL, "multigrid: grid must have 1 to 3 axes");
  n[0] = n[1] = n[2] = 1;
  long prod = 1;
  for (int a = 0; a < ndim; ++a) {
    if (grid[a] < 1) return fail(PSP_EINVAL, "multigrid: grid axes must be positive");
    n[a] = grid[a];
    prod *= grid[a];
    if (prod > 0x7fffffffL) return fail(PSP_EINVAL, "multigrid: prod(grid) does not match the matrix order");
  }
  if (A->nrows != A->ncols) return fail(PSP_EINVAL, "matrix is not square");
  if (prod != A->nrows) return fail(PSP_EINVAL, "multigrid: prod(grid) = %ld does not match the matrix order %d", prod, A->nrows);
  if (!(omega > 0.0 && omega <= 1.0)) return fail(PSP_EINVAL, "multigrid: omega must satisfy 0 < omega <= 1");
  if (steps < 1) return fail(PSP_EINVAL, "multigrid: steps must be >= 1");
  return csr_spmm_check("precon.multigrid", A);
}

// the geometry of the cycle, the same in both modes: the level grids (n, co, nc, rs, N of every level; c, d, w are left
// 0), the first level of the tail and the launches of one application
int mg_level_grids(psp_mg *K, const int n[3], int steps) {
  int cur[3] = {n[0], n[1], n[2]};
  for (;;) {
    psp_mg::Level L;
    memset(&L.a, 0, sizeof L.a);
    int coarsened = 0;
    for (int a = 0; a < 3; ++a) {
      L.a.n[a] = cur[a];
      L.a.co[a] = cur[a] >= 4;
      L.a.nc[a] = L.a.co[a] ? cur[a] / 2 : cur[a];
      coarsened += L.a.co[a];
    }
    L.a.rs = 1.0 / (double)(1 << coarsened);
    L.N = (long)cur[0] * cur[1] * cur[2];
    K->lev.push_back(L);
    if (!coarsened) break;
    for (int a = 0; a < 3; ++a)
      if (L.a.co[a]) cur[a] /= 2;
  }
  const int nl = (int)K->lev.size();
  K->tail_first = nl - 1;
  while (K->tail_first > 0 && K->lev[K->tail_first - 1].N <= kTailT) --K->tail_first;
  // launches of one application: per large level the pre-smoothing (the first two sweeps are one pass), the restriction,
  // the prolongation and the post-smoothing; one for the tail
  K->launches = 1;
  for (int l = 0; l < K->tail_first; ++l) K->launches += (steps >= 2 ? steps - 1 : 1) + 1 + 1 + steps;
  if (nl - K->tail_first > kTailMaxLev || nl > kMaxLevels) return fail(PSP_EINVAL, "multigrid: too many levels");
  return PSP_OK;
}

// level vectors: the finest level works in the caller's vectors and one spare; a level that heads the tail needs its
// b and x in memory (the restriction above it writes b, the prolongation reads x); the levels inside the tail have none
int mg_alloc_vectors(psp_mg *K) {
  for (int l = 0; l <= K->tail_first; ++l) {
    psp_mg::Level &L = K->lev[l];
    const size_t bytes = sizeof(double) * (size_t)L.N;
    hipError_t e = hipSuccess;
    if (l < K->tail_first) e = hipMalloc((void **)&L.t, bytes);
    if (l > 0 && e == hipSuccess) e = hipMalloc((void **)&L.x, bytes);
    if (l > 0 && e == hipSuccess) e = hipMalloc((void **)&L.b, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(PSP_ENOMEM, "multigrid: level vector allocation failed");
    }
  }
  return PSP_OK;
}

// the tail's table (level(l) = what the mode keeps of level l) and the coarsest level's inverse, to the device
template <class LevelOf>
int mg_upload_tail(psp_mg *K, const std::vector<double> &inv, LevelOf &&level) {
  TailArg<std::decay_t<decltype(level(0))>> T;
  memset(&T, 0, sizeof T);
  const int nl = (int)K->lev.size();
  T.nlev = nl - K->tail_first;
  T.steps = K->steps;
  int off = 0;
  for (int l = K->tail_first; l < nl; ++l) {
    T.off[l - K->tail_first] = off;
    T.lev[l - K->tail_first] = level(l);
    off += (int)K->lev[l].N;
  }
  if (off > 2 * kTailT) return fail(PSP_EINVAL, "multigrid: the tail does not fit");
  if (hipMalloc((void **)&K->minv, sizeof(double) * inv.size()) != hipSuccess ||
      hipMalloc(&K->tail, sizeof T) != hipSuccess ||
      hipMemcpy(K->minv, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(K->tail, &T, sizeof T, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PSP_ENOMEM, "multigrid: tail table allocation failed");
  }
  return PSP_OK;
}

// the handle of either mode: build(K) is everything that can fail once it exists (it is destroyed then)
template <class Build>
int mg_make(const psp_csr *A, int ndim, double omega, int steps, bool galerkin, psp_mg **out, Build &&build) {
  psp_mg *K = new psp_mg();
  K->n = A->nrows;
  K->ndim = ndim;
  K->omega = omega;
  K->steps = steps;
  K->galerkin = galerkin;
  const int rc = build(K);
  if (rc != PSP_OK) {
    psp_mg_destroy(K);
    return rc;
  }
  *out = K;
  return PSP_OK;
}

int mg_create(psp_csr *A, int ndim, const int *grid, double omega, int steps, psp_mg **out) {
  int n[3];
  PSP_TRY(mg_check_args(A, ndim, grid, omega, steps, out, n));
  PSP_TRY(ensure_device());
  MgStencil S;
  PSP_TRY(read_stencil(A, n, &S));
  double csum = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (n[a] > 1 && !(S.c[a] > 0.0)) return fail(PSP_EINVAL, "multigrid: the coupling along axis %d is not negative", a);
    csum += S.c[a];
  }
  double s = S.d0 - 2.0 * csum;
  if (!(s >= -16.0 * DBL_EPSILON * std::fabs(S.d0)) || !(S.d0 > 0.0))
    return fail(PSP_EINVAL, "multigrid: the shift s = diagonal - 2 sum c = %g is negative", s);
  if (s < 0.0) s = 0.0;

  return mg_make(A, ndim, omega, steps, false, out, [&](psp_mg *K) {
    // the levels: c_a / 4 on the axes coarsened above, d = 2 sum c + s
    PSP_TRY(mg_level_grids(K, n, steps));
    double c[3] = {S.c[0], S.c[1], S.c[2]};
    for (psp_mg::Level &L : K->lev) {
      double sum = 0.0;
      for (int a = 0; a < 3; ++a) {
        L.a.c[a] = L.a.n[a] > 1 ? c[a] : 0.0;
        sum += L.a.c[a];
      }
      L.a.d = 2.0 * sum + s;
      L.a.w = omega / L.a.d;
      for (int a = 0; a < 3; ++a)
        if (L.a.co[a]) c[a] /= 4.0;
    }
    PSP_TRY(mg_alloc_vectors(K));
    std::vector<double> inv;
    PSP_TRY(coarsest_inverse(K->lev.back().a, &inv));
    return mg_upload_tail(K, inv, [&](int l) { return K->lev[l].a; });
  });
}

// ------------------------------------------------------------------ galerkin = True: creation

const char *g_why(int bits) {
  if (bits & kGBadOffset) return "an entry at an offset that is no axis stride of the grid";
  if (bits & kGBadWrap) return "an entry that wraps across a line end";
  if (bits & kGBadDup) return "an entry that is stored twice";
  if (bits & kGBadDiag) return "a diagonal entry that is missing, or not finite and > 0";
  return "an unsymmetric pair, A[k, k+st] != A[k+st, k]";
}

GOut g_out(const GLevel &G) {
  GOut o;
  o.diag = const_cast<double *>(G.diag);
  o.w = const_cast<double *>(G.w);
  for (int k = 0; k < kGMaxOff; ++k) o.lo[k] = const_cast<double *>(G.lo[k]);
  return o;
}

int g_bad_shape(const GLevel &G) {
  return fail(PSP_EINVAL, "multigrid: internal error (a level of %d axes with %d lower arrays)", G.nd, G.noff);
}

// f(GShape<ND, NOFF>{}) for the level's shape: the one place that turns (nd, noff) into template arguments
template <int ND, int NOFF>
struct GShape {
  static constexpr int nd = ND, noff = NOFF;
};
template <class F>
int g_dispatch(const GLevel &G, F &&f) {
  switch (G.nd * 16 + G.noff) {
    case 1 * 16 + 1: f(GShape<1, 1>{}); break;
    case 2 * 16 + 2: f(GShape<2, 2>{}); break;
    case 2 * 16 + 4: f(GShape<2, 4>{}); break;
    case 3 * 16 + 3: f(GShape<3, 3>{}); break;
    case 3 * 16 + 13: f(GShape<3, 13>{}); break;
    default: return g_bad_shape(G);
  }
  return PSP_OK;
}

int launch_galerkin(const GLevel &S, long Nc, double omega, const GOut &o, int *flag) {
  return g_dispatch(S, [&](auto sh) {
    hipLaunchKernelGGL((mg_galerkin_kernel<sh.nd, sh.noff>), dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, stream(), S,
                       Nc, omega, o, flag);
  });
}

// the dense matrix of a (small) level from its downloaded arrays: blk = diagonal, omega / diagonal, the lower arrays
void g_dense(const GLevel &G, const std::vector<double> &blk, std::vector<double> *M) {
  const int n0 = G.a.n[0], n1 = G.a.n[1], n2 = G.a.n[2], m = n0 * n1 * n2;
  M->assign((size_t)m * m, 0.0);
  for (int r = 0; r < m; ++r) {
    const int g[3] = {r % n0, (r / n0) % n1, r / (n0 * n1)};
    (*M)[(size_t)r * m + r] = blk[r];
    for (int k = 0; k < G.noff; ++k) {
      const int d[3] = {g_d(G.nd, G.noff, k, 0), g_d(G.nd, G.noff, k, 1), g_d(G.nd, G.noff, k, 2)};
      const int h[3] = {g[0] + d[0], g[1] + d[1], g[2] + d[2]};
      if (h[0] < 0 || h[0] >= n0 || h[1] < 0 || h[1] >= n1 || h[2] < 0 || h[2] >= n2) continue;
      const int c = h[0] + n0 * (h[1] + n1 * h[2]);
      const double v = blk[(size_t)(2 + k) * m + r];
      (*M)[(size_t)r * m + c] = v;
      (*M)[(size_t)c * m + r] = v;
    }
  }
}

// mg_create_galerkin's part of mg_make
int g_build(psp_mg *K, const psp_csr *A, const int n[3], int *flags) {
  const double omega = K->omega;
  const int nd = n[2] > 1 ? 3 : n[1] > 1 ? 2 : 1;
  PSP_TRY(mg_level_grids(K, n, K->steps));  // section 9c's
  const int nl = (int)K->lev.size();
  // the level vectors and the level operators' arrays
  PSP_TRY(mg_alloc_vectors(K));
  K->glev.resize(nl);
  K->coef.assign(nl, nullptr);
  for (int l = 0; l < nl; ++l) {
    psp_mg::Level &L = K->lev[l];
    GLevel &G = K->glev[l];
    memset(&G, 0, sizeof G);
    G.a = L.a;
    G.nd = nd;
    G.noff = l == 0 ? nd : g_full_noff(nd);
    if (hipMalloc((void **)&K->coef[l], sizeof(double) * (size_t)(2 + G.noff) * (size_t)L.N) != hipSuccess) {
      (void)hipGetLastError();
      return fail(PSP_ENOMEM, "multigrid: level operator allocation failed");
    }
    G.diag = K->coef[l];
    G.w = K->coef[l] + L.N;
    for (int k = 0; k < G.noff; ++k) {
      G.lo[k] = K->coef[l] + (size_t)(2 + k) * (size_t)L.N;
      for (int a = 0; a < 3; ++a) G.od[k][a] = g_d(nd, G.noff, k, a);
    }
  }
  // level 0: the checking pass writes it
  PSP_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), stream()));
  PSP_HIP(hipMemsetAsync(K->coef[0], 0, sizeof(double) * (size_t)(2 + nd) * (size_t)K->lev[0].N, stream()));
  hipLaunchKernelGGL(mg_extract_csr_kernel, dim3((A->nrows + 255) / 256), dim3(256), 0, stream(), A->nrows, n[0], n[1], n[2],
                     omega, (const int *)A->ind, (const int *)A->col, (const double *)A->val, g_out(K->glev[0]), flags);
  PSP_LAUNCH_CHECK();
  int bad = 0;
  PSP_TRY(read_flag(flags, &bad));
  if (bad)
    return fail(PSP_EINVAL, "multigrid(galerkin=True): the matrix is not a symmetric 3- / 5- / 7-point stencil on this grid: it has %s",
                g_why(bad));
  // A_{l+1} = R_l A_l P_l, level by level
  for (int l = 0; l + 1 < nl; ++l) {
    PSP_TRY(launch_galerkin(K->glev[l], K->lev[l + 1].N, omega, g_out(K->glev[l + 1]), flags + 1));
    PSP_LAUNCH_CHECK();
  }
  PSP_TRY(read_flag(flags + 1, &bad));
  if (bad) return fail(PSP_ESINGULAR, "multigrid(galerkin=True): a level operator's diagonal is not finite and > 0");
  // the coarsest level: downloaded and inverted on the host
  const GLevel &C = K->glev[nl - 1];
  const int m = (int)K->lev[nl - 1].N;
  std::vector<double> blk((size_t)(2 + C.noff) * m), M, inv;
  PSP_HIP(hipMemcpyAsync(blk.data(), K->coef[nl - 1], sizeof(double) * blk.size(), hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  g_dense(C, blk, &M);
  PSP_TRY(dense_inverse(m, M, &inv));
  return mg_upload_tail(K, inv, [&](int l) { return K->glev[l]; });
}

int mg_create_galerkin(psp_csr *A, int ndim, const int *grid, double omega, int steps, psp_mg **out) {
  int n[3];
  PSP_TRY(mg_check_args(A, ndim, grid, omega, steps, out, n));
  if (!(A->ind && A->col && A->val) || A->w4_only)
    return fail(PSP_EINVAL, "multigrid(galerkin=True): the handle no longer holds its index arrays on the device");
  PSP_TRY(ensure_device());
  int *flags = nullptr;
  PSP_HIP(hipMalloc((void **)&flags, 2 * sizeof(int)));
  const int rc = mg_make(A, ndim, omega, steps, true, out, [&](psp_mg *K) { return g_build(K, A, n, flags); });
  (void)hipFree(flags);
  return rc;
}

template <class Op, bool FROMB>
void launch_smooth(const typename Op::Level &A, long N, const double *xin, const double *b, double *xout) {
  hipLaunchKernelGGL((mg_smooth_kernel<Op, FROMB>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream(), A, N, xin, b,
                     xout);
}

template <class Op>
void launch_restrict(const typename Op::Level &A, const double *x, const double *b, double *bc) {
  const MgLevelArg &a = level_geo(A);
  int tile[3];
  mg_tile(a, tile);
  // at most ceil(nc0 / t0) ceil(nc1 / t1) ceil(nc2 / t2) <= 2^31 / 256 + a few tiles: fits gridDim.x
  const long g0n = (a.nc[0] + tile[0] - 1) / tile[0], g1n = (a.nc[1] + tile[1] - 1) / tile[1],
             g2n = (a.nc[2] + tile[2] - 1) / tile[2];
  hipLaunchKernelGGL((mg_restrict_kernel<Op>), dim3((unsigned)(g0n * g1n * g2n)), dim3(kResThreads), 0, stream(), A, tile[0],
                     tile[1], tile[2], (int)g0n, (int)g1n, x, b, bc);
}

// what the steps of the schedule below launch: the first pass from x = 0 (x = w b when steps = 1, else sweeps one and two
// in one pass over b), a further sweep, b_c = R (b - A x), the tail -- the cycle kernels with the mode's policy
struct LevelOps {
  psp_mg *K;
  using Vec = double *;
  Vec lx(int l) const { return K->lev[l].x; }
  Vec lb(int l) const { return K->lev[l].b; }
  Vec lt(int l) const { return K->lev[l].t; }
  void prolong(int l, const double *e, double *x) const {
    const psp_mg::Level &L = K->lev[l];
    hipLaunchKernelGGL(mg_prolong_kernel, dim3((unsigned)((L.N + 255) / 256)), dim3(256), 0, stream(), L.a, L.N, e, x);
  }
  template <bool FROMB>
  int smooth(int l, const double *xin, const double *b, double *xout) const {
    const long N = K->lev[l].N;
    if (K->galerkin) {
      const GLevel &G = K->glev[l];
      return g_dispatch(G, [&](auto sh) { launch_smooth<GOp<sh.nd, sh.noff>, FROMB>(G, N, xin, b, xout); });
    }
    const MgLevelArg &a = K->lev[l].a;
    switch (level_nd(a)) {
      case 1: launch_smooth<MfOp<1>, FROMB>(a, N, xin, b, xout); break;
      case 2: launch_smooth<MfOp<2>, FROMB>(a, N, xin, b, xout); break;
      default: launch_smooth<MfOp<3>, FROMB>(a, N, xin, b, xout); break;
    }
    return PSP_OK;
  }
  int first(int l, const double *b, double *dst) const {
    if (K->steps > 1) return smooth<true>(l, nullptr, b, dst);
    const long N = K->lev[l].N;
    const dim3 g((unsigned)((N + 255) / 256)), t(256);
    if (K->galerkin)
      hipLaunchKernelGGL(mg_scale_kernel<GW>, g, t, 0, stream(), N, GW{K->glev[l].w}, b, dst);
    else
      hipLaunchKernelGGL(mg_scale_kernel<MfW>, g, t, 0, stream(), N, MfW{K->lev[l].a.w}, b, dst);
    return PSP_OK;
  }
  int sweep(int l, const double *xin, const double *b, double *xout) const { return smooth<false>(l, xin, b, xout); }
  int restrict_to(int l, const double *x, const double *b, double *bc) const {
    if (K->galerkin) {
      const GLevel &G = K->glev[l];
      return g_dispatch(G, [&](auto sh) { launch_restrict<GOp<sh.nd, sh.noff>>(G, x, b, bc); });
    }
    launch_restrict<MfOp<3>>(K->lev[l].a, x, b, bc);
    return PSP_OK;
  }
  void tail(const double *b, double *x) const {
    if (K->galerkin)
      hipLaunchKernelGGL(mg_tail_kernel<GTailOp>, dim3(1), dim3(kTailThreads), 0, stream(),
                         (const TailArg<GLevel> *)K->tail, (const double *)K->minv, b, x);
    else
      hipLaunchKernelGGL(mg_tail_kernel<MfOp<3>>, dim3(1), dim3(kTailThreads), 0, stream(),
                         (const TailArg<MgLevelArg> *)K->tail, (const double *)K->minv, b, x);
  }
};

// a block of vectors: column c at p + c * ld
struct BVec {
  double *p = nullptr;
  long ld = 0;
  const double *cp() const { return p; }
  bool operator==(const BVec &o) const { return p == o.p; }
  bool operator!=(const BVec &o) const { return p != o.p; }
};

// Columns per thread of the block kernels, by measurement (DESIGN.md section 9e has the register table and the figures).
// The sweep, scale and prolongation kernels take groups of four columns with stored level operators, whose row of up to 27
// coefficients is then loaded once for four columns, and of two in the matrix-free mode, which has nothing to share
// but the index split (two where k <= 2 in both).  The restriction takes ONE column per workgroup (kBlockKCR = 1, the
// columns in gridDim.y): holding 2 or 4 residual tiles in LDS to share the rows was 5 to 22 % and 40 to 70 % slower.
constexpr int kBlockKCGalerkin = 4;
constexpr int kBlockKCMatrixFree = 2;
constexpr int kBlockKCR = 1;
// op_apply_block and psp_pcg_batch run the block cycle in these modes (section 9e's routing decision)
constexpr bool kRouteBlockMatrixFree = true;
constexpr bool kRouteBlockGalerkin = true;

int block_tuning(const char *name, int dflt, std::initializer_list<int> allowed) {
  const char *e = tuning_env(name);
  if (!e) return dflt;
  const int v = atoi(e);
  for (int a : allowed)
    if (a == v) return v;
  return dflt;
}

// the block cycle's launches: LevelOps with the column count, the leading dimensions and the frozen flags
struct BlockOps {
  psp_mg *K;
  int k;
  const int *frozen;
  int kc, kcr;
  using Vec = BVec;
  BlockOps(psp_mg *K_, int k_, const int *frozen_) : K(K_), k(k_), frozen(frozen_) {
    kc = k <= 2 ? 2 : block_tuning("PSP_MG_BLOCK_KC", K->galerkin ? kBlockKCGalerkin : kBlockKCMatrixFree, {2, 4});
    kcr = k == 1 ? 1 : block_tuning("PSP_MG_BLOCK_KCR", kBlockKCR, {1, 2, 4});
  }
  Vec lx(int l) const { return BVec{K->blk[l].x, K->lev[l].N}; }
  Vec lb(int l) const { return BVec{K->blk[l].b, K->lev[l].N}; }
  Vec lt(int l) const { return BVec{K->blk[l].t, K->lev[l].N}; }
  dim3 grid(long N) const { return dim3((unsigned)((N + 255) / 256), (unsigned)((k + kc - 1) / kc)); }

  template <class Op, bool FROMB>
  void launch_smooth(const typename Op::Level &A, long N, BVec xin, BVec b, BVec xout) const {
    if (kc == 4)
      hipLaunchKernelGGL((mg_smooth_block_kernel<Op, FROMB, 4>), grid(N), dim3(256), 0, stream(), A, N, k, xin.cp(), xin.ld,
                         b.cp(), b.ld, xout.p, xout.ld, frozen);
    else
      hipLaunchKernelGGL((mg_smooth_block_kernel<Op, FROMB, 2>), grid(N), dim3(256), 0, stream(), A, N, k, xin.cp(), xin.ld,
                         b.cp(), b.ld, xout.p, xout.ld, frozen);
  }
  template <bool FROMB>
  int smooth(int l, BVec xin, BVec b, BVec xout) const {
    const long N = K->lev[l].N;
    if (K->galerkin) {
      const GLevel &G = K->glev[l];
      return g_dispatch(G, [&](auto sh) { launch_smooth<GOp<sh.nd, sh.noff>, FROMB>(G, N, xin, b, xout); });
    }
    const MgLevelArg &a = K->lev[l].a;
    switch (level_nd(a)) {
      case 1: launch_smooth<MfOp<1>, FROMB>(a, N, xin, b, xout); break;
      case 2: launch_smooth<MfOp<2>, FROMB>(a, N, xin, b, xout); break;
      default: launch_smooth<MfOp<3>, FROMB>(a, N, xin, b, xout); break;
    }
    return PSP_OK;
  }
  template <class W>
  void launch_scale(long N, W w, BVec b, BVec dst) const {
    if (kc == 4)
      hipLaunchKernelGGL((mg_scale_block_kernel<W, 4>), grid(N), dim3(256), 0, stream(), N, w, k, b.cp(), b.ld, dst.p, dst.ld,
                         frozen);
    else
      hipLaunchKernelGGL((mg_scale_block_kernel<W, 2>), grid(N), dim3(256), 0, stream(), N, w, k, b.cp(), b.ld, dst.p, dst.ld,
                         frozen);
  }
  int first(int l, BVec b, BVec dst) const {
    if (K->steps > 1) return smooth<true>(l, BVec(), b, dst);
    const long N = K->lev[l].N;
    if (K->galerkin)
      launch_scale(N, GW{K->glev[l].w}, b, dst);
    else
      launch_scale(N, MfW{K->lev[l].a.w}, b, dst);
    return PSP_OK;
  }
  int sweep(int l, BVec xin, BVec b, BVec xout) const { return smooth<false>(l, xin, b, xout); }

  template <class Op, int KCR>
  void launch_restrict_kc(const typename Op::Level &A, BVec x, BVec b, BVec bc) const {
    const MgLevelArg &a = level_geo(A);
    int tile[3];
    mg_tile(a, tile);
    const long g0n = (a.nc[0] + tile[0] - 1) / tile[0], g1n = (a.nc[1] + tile[1] - 1) / tile[1],
               g2n = (a.nc[2] + tile[2] - 1) / tile[2];
    hipLaunchKernelGGL((mg_restrict_block_kernel<Op, KCR>), dim3((unsigned)(g0n * g1n * g2n), (unsigned)((k + KCR - 1) / KCR)),
                       dim3(kResThreads), 0, stream(), A, tile[0], tile[1], tile[2], (int)g0n, (int)g1n, k, x.cp(), x.ld,
                       b.cp(), b.ld, bc.p, bc.ld, frozen);
  }
  template <class Op>
  void launch_restrict(const typename Op::Level &A, BVec x, BVec b, BVec bc) const {
    if (kcr == 4)
      launch_restrict_kc<Op, 4>(A, x, b, bc);
    else if (kcr == 2)
      launch_restrict_kc<Op, 2>(A, x, b, bc);
    else
      launch_restrict_kc<Op, 1>(A, x, b, bc);
  }
  int restrict_to(int l, BVec x, BVec b, BVec bc) const {
    if (K->galerkin) {
      const GLevel &G = K->glev[l];
      return g_dispatch(G, [&](auto sh) { launch_restrict<GOp<sh.nd, sh.noff>>(G, x, b, bc); });
    }
    launch_restrict<MfOp<3>>(K->lev[l].a, x, b, bc);
    return PSP_OK;
  }
  void tail(BVec b, BVec x) const {
    if (K->galerkin)
      hipLaunchKernelGGL(mg_tail_block_kernel<GTailOp>, dim3(k), dim3(kTailThreads), 0, stream(),
                         (const TailArg<GLevel> *)K->tail, (const double *)K->minv, b.cp(), b.ld, x.p, x.ld, frozen);
    else
      hipLaunchKernelGGL(mg_tail_block_kernel<MfOp<3>>, dim3(k), dim3(kTailThreads), 0, stream(),
                         (const TailArg<MgLevelArg> *)K->tail, (const double *)K->minv, b.cp(), b.ld, x.p, x.ld, frozen);
  }
  void prolong(int l, BVec e, BVec x) const {
    const psp_mg::Level &L = K->lev[l];
    if (kc == 4)
      hipLaunchKernelGGL(mg_prolong_block_kernel<4>, grid(L.N), dim3(256), 0, stream(), L.a, L.N, k, e.cp(), e.ld, x.p, x.ld,
                         frozen);
    else
      hipLaunchKernelGGL(mg_prolong_block_kernel<2>, grid(L.N), dim3(256), 0, stream(), L.a, L.N, k, e.cp(), e.ld, x.p, x.ld,
                         frozen);
  }
};

// the sss entry points: an sss_mat is read through its full device mirror
int mg_create_sss(psp_sss_t *A, const char *fn, int (*create)(psp_csr *, int, const int *, double, int, psp_mg **), int ndim,
                  const int *grid, double omega, int steps, psp_mg **out) {
  PSP_API_GUARD_H(A, A ? A->full : nullptr);
  if (!A) return fail(PSP_EINVAL, "%s: NULL argument", fn);
  if (A->host || cpu_mode())
    return fail(PSP_ENODEV, "precon.multigrid: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  if (!A->full) return fail(PSP_EINVAL, "%s: the matrix has no device mirror", fn);
  return create(A->full, ndim, grid, omega, steps, out);
}

// one V-cycle: the schedule of launches and buffers, the same in both modes and for one vector (Ops::Vec = double *) or a
// block of them (BVec): K->launches launches whatever the column count is.  b_dev is only read.
template <class Ops>
int mg_schedule(psp_mg *K, typename Ops::Vec b_dev, typename Ops::Vec y_dev, const Ops &ops) {
  using V = typename Ops::Vec;
  const int steps = K->steps, tf = K->tail_first;
  // where each large level's iterate is after its pre-smoothing; every sweep writes the buffer the previous one did not
  V cur[kMaxLevels] = {};
  // down
  for (int l = 0; l < tf; ++l) {
    const V b = l == 0 ? b_dev : ops.lb(l);
    const V own = l == 0 ? y_dev : ops.lx(l);
    // the finest level's last sweep must land in y: its writes are the pre-smoothing launches and `steps` more
    const int writes = (steps >= 2 ? steps - 1 : 1) + steps;
    V dst = (l == 0 && (writes & 1) == 0) ? ops.lt(l) : own;
    PSP_TRY(ops.first(l, b, dst));
    for (int k = 2; k < steps; ++k) {
      V nxt = dst == own ? ops.lt(l) : own;
      PSP_TRY(ops.sweep(l, dst, b, nxt));
      dst = nxt;
    }
    cur[l] = dst;
    PSP_TRY(ops.restrict_to(l, dst, b, ops.lb(l + 1)));
    PSP_LAUNCH_CHECK();
  }
  // the tail
  {
    const V b = tf == 0 ? b_dev : ops.lb(tf);
    V x = tf == 0 ? y_dev : ops.lx(tf);
    ops.tail(b, x);
    PSP_LAUNCH_CHECK();
    cur[tf] = x;
  }
  // up
  for (int l = tf - 1; l >= 0; --l) {
    const V b = l == 0 ? b_dev : ops.lb(l);
    const V own = l == 0 ? y_dev : ops.lx(l);
    V x = cur[l];
    ops.prolong(l, cur[l + 1], x);
    for (int k = 0; k < steps; ++k) {
      V nxt = x == own ? ops.lt(l) : own;
      PSP_TRY(ops.sweep(l, x, b, nxt));
      x = nxt;
    }
    cur[l] = x;
    PSP_LAUNCH_CHECK();
  }
  if (tf > 0 && cur[0] != y_dev) return fail(PSP_EINVAL, "multigrid: internal error (the result is not in y)");
  return PSP_OK;
}

void mg_block_free(psp_mg *K) {
  for (psp_mg::BlockLevel &B : K->blk)
    for (void *p : {(void *)B.x, (void *)B.b, (void *)B.t}) (void)hipFree(p);
  K->blk.clear();
  K->blk_cols = 0;
  K->blk_bytes = 0;
}

// the block cycle's level vectors for at least k columns (k = 0: none); what mg_alloc_vectors allocates, k columns wide.
// hipFree waits for the device, so nothing that still runs loses its buffers.
int mg_block_reserve(psp_mg *K, int k) {
  if (k == 0) {
    mg_block_free(K);
    return PSP_OK;
  }
  if (k <= K->blk_cols) return PSP_OK;
  mg_block_free(K);
  K->blk.resize(K->lev.size());
  for (int l = 0; l <= K->tail_first; ++l) {
    psp_mg::BlockLevel &B = K->blk[l];
    const size_t bytes = sizeof(double) * (size_t)K->lev[l].N * (size_t)k;
    hipError_t e = hipSuccess;
    size_t got = 0;
    if (l < K->tail_first) e = hipMalloc((void **)&B.t, bytes), got += e == hipSuccess ? bytes : 0;
    if (l > 0 && e == hipSuccess) e = hipMalloc((void **)&B.x, bytes), got += e == hipSuccess ? bytes : 0;
    if (l > 0 && e == hipSuccess) e = hipMalloc((void **)&B.b, bytes), got += e == hipSuccess ? bytes : 0;
    K->blk_bytes += got;
    if (e != hipSuccess) {
      (void)hipGetLastError();
      mg_block_free(K);
      return fail(PSP_ENOMEM, "multigrid: block level vector allocation failed (%d columns)", k);
    }
  }
  K->blk_cols = k;
  return PSP_OK;
}

}  // namespace

namespace psp {

// y = V(0, b) on device vectors; y must not alias b.  The handle is locked by the caller.
int mg_apply_dev(psp_mg *K, const double *b_dev, double *y_dev) {
  return mg_schedule(K, const_cast<double *>(b_dev), y_dev, LevelOps{K});
}

// Y[:, c] = V(0, X[:, c]) for every column c < k with frozen[c] == 0 (frozen == nullptr: every column), one block cycle:
// the bits of mg_apply_dev on the column, K's launches whatever k is.  Y must not overlap X.  The handle is locked by the
// caller.
int mg_apply_block_dev(psp_mg *K, int k, const double *X, long ldx, double *Y, long ldy, const int *frozen) {
  PSP_TRY(mg_block_reserve(K, k));
  return mg_schedule(K, BVec{const_cast<double *>(X), ldx}, BVec{Y, ldy}, BlockOps(K, k, frozen));
}

int mg_launches(const psp_mg *K) { return K->launches; }

// Where op_apply_block and the batched PCG loop run the block cycle and where they keep the column-by-column path: by the
// measurements of DESIGN.md section 9e (profiles/mg_block_timing.json).
bool mg_block_routed(const psp_mg *K) { return K->galerkin ? kRouteBlockGalerkin : kRouteBlockMatrixFree; }

}  // namespace psp

extern "C" {

int psp_mg_create_csr(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  PSP_API_GUARD_H(A);
  return mg_create(A, ndim, grid, omega, steps, out);
}

int psp_mg_create_sss(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return mg_create_sss(A, "psp_mg_create_sss", mg_create, ndim, grid, omega, steps, out);
}

int psp_mg_create_csr_galerkin(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  PSP_API_GUARD_H(A);
  return mg_create_galerkin(A, ndim, grid, omega, steps, out);
}

int psp_mg_create_sss_galerkin(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return mg_create_sss(A, "psp_mg_create_sss_galerkin", mg_create_galerkin, ndim, grid, omega, steps, out);
}

int psp_mg_is_galerkin(const psp_mg_t *K, int *galerkin) {
  if (!K || !galerkin) return fail(PSP_EINVAL, "psp_mg_is_galerkin: NULL argument");
  *galerkin = K->galerkin ? 1 : 0;
  return PSP_OK;
}

int psp_mg_level_operator(psp_mg_t *K, int level, int *offsets_out, int *noff_inout, double *values_host) {
  PSP_API_GUARD_H(K);
  if (!K || !noff_inout) return fail(PSP_EINVAL, "psp_mg_level_operator: NULL argument");
  if (!K->galerkin) return fail(PSP_EINVAL, "psp_mg_level_operator: the handle stores no level operators (galerkin=False)");
  if (level < 0 || level >= (int)K->glev.size()) return fail(PSP_EINVAL, "psp_mg_level_operator: no level %d", level);
  const GLevel &G = K->glev[level];
  const int cap = *noff_inout, cnt = 1 + G.noff;
  *noff_inout = cnt;
  if (!offsets_out && !values_host) return PSP_OK;
  if (cap < cnt) return fail(PSP_EINVAL, "psp_mg_level_operator: room for %d arrays, the level has %d", cap, cnt);
  if (offsets_out) {
    offsets_out[0] = offsets_out[1] = offsets_out[2] = 0;
    for (int k = 0; k < G.noff; ++k)
      for (int a = 0; a < 3; ++a) offsets_out[3 * (k + 1) + a] = g_d(G.nd, G.noff, k, a);
  }
  if (values_host) {
    const size_t N = (size_t)K->lev[level].N;
    PSP_TRY(ensure_device());
    PSP_HIP(hipMemcpyAsync(values_host, G.diag, sizeof(double) * N, hipMemcpyDeviceToHost, stream()));
    if (G.noff > 0)  // the lower arrays follow omega / diagonal in the level's allocation
      PSP_HIP(hipMemcpyAsync(values_host + N, G.lo[0], sizeof(double) * N * (size_t)G.noff, hipMemcpyDeviceToHost, stream()));
    PSP_HIP(hipStreamSynchronize(stream()));
  }
  return PSP_OK;
}

int psp_mg_destroy(psp_mg_t *K) {
  if (!K) return PSP_OK;
  mg_block_free(K);
  for (double *p : K->coef) (void)hipFree(p);
  for (psp_mg::Level &L : K->lev)
    for (void *p : {(void *)L.x, (void *)L.b, (void *)L.t}) (void)hipFree(p);
  (void)hipFree(K->minv);
  (void)hipFree(K->tail);
  delete K;
  return PSP_OK;
}

int psp_mg_info(const psp_mg_t *K, int *levels, int *tail_first_level, int *launches_per_apply, int *dims) {
  if (!K) return fail(PSP_EINVAL, "psp_mg_info: NULL handle");
  if (levels) *levels = (int)K->lev.size();
  if (tail_first_level) *tail_first_level = K->tail_first;
  if (launches_per_apply) *launches_per_apply = K->launches;
  if (dims)
    for (size_t l = 0; l < K->lev.size(); ++l)
      for (int a = 0; a < 3; ++a) dims[3 * l + a] = K->lev[l].a.n[a];
  return PSP_OK;
}

int psp_op_from_mg(psp_mg_t *K, psp_op_t **out) {
  if (!K || !out) return fail(PSP_EINVAL, "psp_op_from_mg: NULL argument");
  psp_op *op = new psp_op();
  op->kind = PSP_OP_MG;
  op->n = K->n;
  op->mg = K;
  *out = op;
  return PSP_OK;
}

int psp_mg_precon_dev(psp_mg_t *K, const double *x_dev, double *y_dev) {
  PSP_API_GUARD_H(K);
  if (!K || !x_dev || !y_dev) return fail(PSP_EINVAL, "psp_mg_precon_dev: NULL argument");
  if (x_dev == y_dev) return fail(PSP_EINVAL, "psp_mg_precon_dev: y must not alias x");
  return mg_apply_dev(K, x_dev, y_dev);
}

int psp_mg_precon(psp_mg_t *K, const double *x_host, double *y_host) {
  PSP_API_GUARD_H(K);
  if (!K || !x_host || !y_host) return fail(PSP_EINVAL, "psp_mg_precon: NULL argument");
  PSP_TRY(ensure_device());
  const size_t n = (size_t)K->n, bytes = sizeof(double) * n;
  double *x = nullptr, *y = nullptr;
  PSP_TRY(scratch_get(n, &x));
  int rc = scratch_get(n, &y);
  if (rc != PSP_OK) {
    scratch_put(x, n);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(x, x_host, bytes, hipMemcpyHostToDevice, stream());
  if (e == hipSuccess) rc = mg_apply_dev(K, x, y);
  if (e == hipSuccess && rc == PSP_OK) e = hipMemcpyAsync(y_host, y, bytes, hipMemcpyDeviceToHost, stream());
  const hipError_t e2 = hipStreamSynchronize(stream());
  scratch_put(x, n);
  scratch_put(y, n);
  if (rc != PSP_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(PSP_ENODEV, "psp_mg_precon: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return PSP_OK;
}

int psp_mg_precon_block_dev(psp_mg_t *K, int k, const double *X_dev, long ldx, double *Y_dev, long ldy) {
  PSP_API_GUARD_H(K);
  if (cpu_mode()) return fail(PSP_ENODEV, "psp_mg_precon_block_dev: not available with PSP_DEVICE=cpu");
  if (!K) return fail(PSP_EINVAL, "psp_mg_precon_block_dev: NULL handle");
  PSP_TRY(block_args("psp_mg_precon_block_dev", K->n, K->n, k, X_dev, ldx, Y_dev, ldy));
  PSP_TRY(ensure_device());
  return mg_apply_block_dev(K, k, X_dev, ldx, Y_dev, ldy, nullptr);
}

int psp_mg_precon_block(psp_mg_t *K, int k, const double *X_host, long ldx, double *Y_host, long ldy) {
  PSP_API_GUARD_H(K);
  if (cpu_mode()) return fail(PSP_ENODEV, "psp_mg_precon_block: not available with PSP_DEVICE=cpu");
  if (!K) return fail(PSP_EINVAL, "psp_mg_precon_block: NULL handle");
  PSP_TRY(block_args("psp_mg_precon_block", K->n, K->n, k, X_host, ldx, Y_host, ldy));
  PSP_TRY(ensure_device());
  const size_t n = (size_t)K->n, nk = n * (size_t)k, row = sizeof(double) * n;
  double *x = nullptr, *y = nullptr;
  PSP_TRY(scratch_get(nk, &x));
  int rc = scratch_get(nk, &y);
  if (rc != PSP_OK) {
    scratch_put(x, nk);
    return rc;
  }
  hipError_t e = hipMemcpy2DAsync(x, row, X_host, sizeof(double) * ldx, row, k, hipMemcpyHostToDevice, stream());
  if (e == hipSuccess) rc = mg_apply_block_dev(K, k, x, (long)n, y, (long)n, nullptr);
  if (e == hipSuccess && rc == PSP_OK)
    e = hipMemcpy2DAsync(Y_host, sizeof(double) * ldy, y, row, row, k, hipMemcpyDeviceToHost, stream());
  const hipError_t e2 = hipStreamSynchronize(stream());
  scratch_put(x, nk);
  scratch_put(y, nk);
  if (rc != PSP_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(PSP_ENODEV, "psp_mg_precon_block: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  return PSP_OK;
}

int psp_mg_block_reserve(psp_mg_t *K, int k) {
  PSP_API_GUARD_H(K);
  if (cpu_mode()) return fail(PSP_ENODEV, "psp_mg_block_reserve: not available with PSP_DEVICE=cpu");
  if (!K) return fail(PSP_EINVAL, "psp_mg_block_reserve: NULL handle");
  if (k < 0) return fail(PSP_EINVAL, "psp_mg_block_reserve: k = %d columns", k);
  PSP_TRY(ensure_device());
  return mg_block_reserve(K, k);
}

int psp_mg_block_info(psp_mg_t *K, int *columns, long long *bytes) {
  PSP_API_GUARD_H(K);
  if (!K) return fail(PSP_EINVAL, "psp_mg_block_info: NULL handle");
  if (columns) *columns = K->blk_cols;
  if (bytes) *bytes = (long long)K->blk_bytes;
  return PSP_OK;
}

}  // extern "C"
