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
// line = a (psp_mg_create_*_line; psp_mg_line.h) is the stored mode with a line smoother for grids
// graded or stretched along axis a: that axis is never coarsened, every other one is halved down to a single point, a
// sweep is x <- x + omega T_l^-1 (b - A_l x) with T_l the tridiagonal part of A_l along the grid lines of axis a (one
// thread per line, factorised at creation), and the last level, a single line, is solved exactly.  The schedule, the
// restriction and the prolongation are the ones below; there is no tail launch and no dense inverse.
//
// stencil = 'box' (PSP_MG_BOX; psp_mg_galerkin.h) is the stored mode for symmetric operators with the full
// pattern {-1, 0, 1}^ND, 9 points in 2-D and 27 in 3-D: a checking and extraction pass of its own, level 0 stored like every
// lower level, the Galerkin chain summed without losing its rounding errors; the cycle kernels are the ones below.
//
// interp = 'operator' (PSP_MG_INTERP; psp_mg_interp.h) is the stored mode with transfers derived from each
// level's own stencil, for coefficients that jump between regions: weights per level, a weighted Galerkin product,
// restriction and prolongation kernels of its own; the smoother kernels are the ones below.  Every level is launches, the
// dense coarsest product one more: there is no tail launch.
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
// LDS of the tail (elements of the cycle's scalar type): x and b of every level (level sizes at least halve: their sum stays below 2 kTailT), one
// level-sized scratch for the residual, the dense inverse
constexpr int kTailLds = 5 * kTailT + kCoarsestMax * kCoarsestMax;
// mg_restrict: 256 coarse points per workgroup; the fine residuals of the tile plus halo (2 t + 1 per coarsened axis)
constexpr int kResThreads = 256;
constexpr int kResLds = 33 * 9 * 9;  // the 3-D tile 16 x 4 x 4; 2-D 32 x 8 -> 65 x 17, 1-D 256 -> 513 are smaller

// S: the scalar type the cycle runs in -- double, or float for precision='single' (the level's
// numbers are formed in double and rounded once)
template <class S>
struct MgLevelArgT {
  int n[3];   // dimensions (1 on the axes the grid does not have)
  int co[3];  // 1: the axis is coarsened towards the next level
  int nc[3];  // dimensions of the next level
  S c[3];     // 0 on axes of length 1
  S d;        // 2 sum c + s
  S w;        // omega / d
  S rs;       // 1 / 2^(coarsened axes)
};
using MgLevelArg = MgLevelArgT<double>;

template <class LevelT>  // what the mode keeps of a level: MgLevelArg, or psp_mg_galerkin.h's GLevel
struct TailArg {
  int nlev;
  int steps;
  int off[kTailMaxLev];  // offset of the level's x (and, kTailT * 2 further, b) in the tail's LDS
  LevelT lev[kTailMaxLev];
};

// (A_l x)[i]: the diagonal first, then axis by axis the lower and the upper neighbour -- one fixed order everywhere
template <class S, class X>
__device__ __forceinline__ S mg_ax(const MgLevelArgT<S> &L, const X &x, long i, int i0, int i1, int i2) {
  S acc = L.d * x(i);
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
template <int ND = 3, class S>
__device__ __forceinline__ void mg_split(const MgLevelArgT<S> &L, long i, int &i0, int &i1, int &i2) {
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
template <int ND, class S>
struct MfOp {
  using Scalar = S;
  static constexpr bool kFinest = true;  // the shape can be the finest level's (mg_with_io)
  using Level = MgLevelArgT<S>;
  Level L;
  __device__ __forceinline__ explicit MfOp(const Level &a) : L(a) {
    if constexpr (ND < 3) L.n[2] = 1;
    if constexpr (ND < 2) L.n[1] = 1;
  }
  __device__ __forceinline__ const Level &geo() const { return L; }
  template <class X>
  __device__ __forceinline__ S ax(const X &x, long i, int i0, int i1, int i2) const {
    return mg_ax(L, x, i, i0, i1, i2);
  }
  __device__ __forceinline__ S w(long) const { return L.w; }
  __device__ __forceinline__ void split(long i, int &i0, int &i1, int &i2) const { mg_split<ND>(L, i, i0, i1, i2); }
  // the block kernels' pair (GOp in psp_mg_galerkin.h has the real one): this mode's row is kernel arguments, nothing is
  // loaded; x(j, w_j) is the column's value at j
  struct Row {
    S w;
  };
  template <bool WN>
  __device__ __forceinline__ Row load_row(long, int, int, int) const {
    return Row{L.w};
  }
  template <class X>
  __device__ __forceinline__ S ax_row(const Row &r, const X &x, long i, int i0, int i1, int i2) const {
    auto X1 = [&](long j) { return x(j, r.w); };
    return mg_ax(L, X1, i, i0, i1, i2);
  }
};
// omega / d as mg_scale_kernel takes it
template <class S>
struct MfW {
  using Scalar = S;
  S w;
  __device__ __forceinline__ S operator()(long) const { return w; }
};
template <class S>
__host__ __device__ inline const MgLevelArgT<S> &level_geo(const MgLevelArgT<S> &a) {
  return a;
}

// (R r)[j] for the coarse point (j0, j1, j2); r is indexed through `at(l0, l1, l2)` with fine coordinates, which returns 0
// outside the grid.  Weights 1/2, 1, 1/2 along a coarsened axis at fine 2j, 2j+1, 2j+2; axis 2 outermost, ascending.
template <class S, class AT>
__device__ __forceinline__ S mg_restrict_point(const MgLevelArgT<S> &L, const AT &at, int j0, int j1, int j2) {
  const int b0 = L.co[0] ? 2 * j0 : j0, m0 = L.co[0] ? 3 : 1;
  const int b1 = L.co[1] ? 2 * j1 : j1, m1 = L.co[1] ? 3 : 1;
  const int b2 = L.co[2] ? 2 * j2 : j2, m2 = L.co[2] ? 3 : 1;
  S sum = 0;
  for (int k2 = 0; k2 < m2; ++k2) {
    const S w2 = (L.co[2] && k2 != 1) ? S(0.5) : S(1);
    for (int k1 = 0; k1 < m1; ++k1) {
      const S w1 = (L.co[1] && k1 != 1) ? S(0.5) * w2 : w2;
      for (int k0 = 0; k0 < m0; ++k0) {
        const S w0 = (L.co[0] && k0 != 1) ? S(0.5) * w1 : w1;
        sum += w0 * at(b0 + k0, b1 + k1, b2 + k2);
      }
    }
  }
  return sum * L.rs;
}

// (P e)[i] for the fine point (i0, i1, i2); e is the next level's vector.  Along a coarsened axis an odd index takes
// coarse (i - 1) / 2 whole, an even one half of coarse i / 2 - 1 and half of i / 2 where they exist; lower before upper,
// axis 2 outermost.
template <class S>
struct MgAxisSrc {
  int ja, jb, cnt;  // the coarse indices a fine index takes from (jb only when cnt == 2)
  S wt;
};
template <class S>
__device__ __forceinline__ MgAxisSrc<S> mg_axis_src(int co, int g, int nc) {
  MgAxisSrc<S> s;
  s.jb = 0;
  if (!co) {
    s.ja = g, s.cnt = 1, s.wt = S(1);
  } else if (g & 1) {
    s.ja = (g - 1) >> 1, s.cnt = 1, s.wt = S(1);
  } else {
    const int lo = (g >> 1) - 1, hi = g >> 1;  // at least one exists: nc >= 2 on a coarsened axis
    s.wt = S(0.5);
    if (lo >= 0 && hi < nc) {
      s.ja = lo, s.jb = hi, s.cnt = 2;
    } else {
      s.ja = lo >= 0 ? lo : hi, s.cnt = 1;
    }
  }
  return s;
}
template <class S, class E>
__device__ __forceinline__ S mg_prolong_point(const MgLevelArgT<S> &L, const E &e, int i0, int i1, int i2) {
  const MgAxisSrc<S> a0 = mg_axis_src<S>(L.co[0], i0, L.nc[0]), a1 = mg_axis_src<S>(L.co[1], i1, L.nc[1]),
                     a2 = mg_axis_src<S>(L.co[2], i2, L.nc[2]);
  const S w = a0.wt * a1.wt * a2.wt;  // powers of two: exact
  S sum = 0;
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

// Element types.  S = the policy's Scalar is what every level vector holds and every operation is done in.  The finest
// level alone also touches the caller's vectors, which are double whatever S is: TB (of b) and TO (of the vector a sweep
// writes) are deduced from the pointers; an element is converted to S as it is loaded, a result to TO as it is stored.
// With S = double all three are double and the conversions are none.

// the first sweep from x = 0: x = 0 + (omega / d)(b - 0) = (omega / d) b; W: MfW (a scalar) or GW (an array)
template <class W, class TB>
__global__ __launch_bounds__(256) void mg_scale_kernel(long N, W w, const TB *__restrict__ b,
                                                       typename W::Scalar *__restrict__ x) {
  using S = typename W::Scalar;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < N) x[i] = w(i) * (S)b[i];
}

// one sweep, out of place: xout = xin + (omega / d)(b - A xin); reads xin and b (and, with a stored stencil, w and every
// coefficient array) once, writes xout once; the neighbours (of xin, and the neighbours' rows of the lower arrays: the
// upper couplings) come from the caches.  FROMB: xin is the first sweep's (omega / d) b, formed on the fly -- sweeps one
// and two of a cycle in one pass.
template <class Op, bool FROMB, class TB, class TO>
__global__ __launch_bounds__(256) void mg_smooth_kernel(typename Op::Level A, long N,
                                                        const typename Op::Scalar *__restrict__ xin,
                                                        const TB *__restrict__ b, TO *__restrict__ xout) {
  using S = typename Op::Scalar;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const Op op(A);
  int i0, i1, i2;
  op.split(i, i0, i1, i2);
  auto X = [&](long k) -> S { return FROMB ? op.w(k) * (S)b[k] : xin[k]; };
  const S ax = op.ax(X, i, i0, i1, i2);
  xout[i] = (TO)(X(i) + op.w(i) * ((S)b[i] - ax));
}

// b_c = R (b - A x): blockIdx.x = the tile of coarse points (t[0] x t[1] x t[2] = 256 of them), `r` = the fine residuals
// the tile's restriction reads; a fine point outside the grid counts as 0.  The fine residual never reaches memory.
template <class Op, class TB>
__global__ __launch_bounds__(kResThreads) void mg_restrict_kernel(typename Op::Level A, int t0, int t1, int t2, int g0n,
                                                                  int g1n, const typename Op::Scalar *__restrict__ x,
                                                                  const TB *__restrict__ b,
                                                                  typename Op::Scalar *__restrict__ bc) {
  using S = typename Op::Scalar;
  __shared__ S r[kResLds];
  const Op op(A);
  const MgLevelArgT<S> &L = op.geo();
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
    S v = 0;
    if (g0 < L.n[0] && g1 < L.n[1] && g2 < L.n[2]) {
      const long i = g0 + (long)L.n[0] * (g1 + (long)L.n[1] * g2);
      v = (S)b[i] - op.ax(X, i, g0, g1, g2);
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
      const S v = mg_restrict_point(L, at, j0, j1, j2);
      bc[(J0 + j0) + (long)L.nc[0] * ((J1 + j1) + (long)L.nc[1] * (J2 + j2))] = v;
    }
  }
}

// x += P e: reads x and e, writes x
template <class S>
__global__ __launch_bounds__(256) void mg_prolong_kernel(MgLevelArgT<S> L, long N, const S *__restrict__ e,
                                                         S *__restrict__ x) {
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

template <class W, int KC, class TB>
__global__ __launch_bounds__(256) void mg_scale_block_kernel(long N, W w, int k, const TB *__restrict__ b, long ldb,
                                                             typename W::Scalar *__restrict__ x, long ldx,
                                                             const int *__restrict__ frozen) {
  using S = typename W::Scalar;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int c0 = blockIdx.y * KC;
  const unsigned live = mg_live<KC>(c0, k, frozen);
  if (i >= N || !live) return;
  const S wi = w(i);
#pragma unroll
  for (int c = 0; c < KC; ++c)
    if ((live >> c) & 1u) x[(size_t)(c0 + c) * ldx + i] = wi * (S)b[(size_t)(c0 + c) * ldb + i];
}

template <class Op, bool FROMB, int KC, class TB, class TO>
__global__ __launch_bounds__(256) void mg_smooth_block_kernel(typename Op::Level A, long N, int k,
                                                              const typename Op::Scalar *__restrict__ xin, long ldi,
                                                              const TB *__restrict__ b, long ldb,
                                                              TO *__restrict__ xout, long ldo,
                                                              const int *__restrict__ frozen) {
  using S = typename Op::Scalar;
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
    const TB *__restrict__ bc = b + (size_t)(c0 + c) * ldb;
    const S *__restrict__ xc = FROMB ? nullptr : xin + (size_t)(c0 + c) * ldi;
    auto X = [&](long j, S wj) -> S {
      if constexpr (FROMB)
        return wj * (S)bc[j];
      else
        return xc[j];
    };
    const S ax = op.ax_row(row, X, i, i0, i1, i2);
    xout[(size_t)(c0 + c) * ldo + i] = (TO)(X(i, row.w) + row.w * ((S)bc[i] - ax));
  }
}

// b_c = R (b - A x), one column per workgroup: blockIdx.y = the column, blockIdx.x = its tile as in mg_restrict_kernel.
// The row of a fine point comes through load_row / ax_row like the other block kernels' (holding 2 or 4 columns' residual
// tiles in LDS to share the rows was measured slower in every row of section 9e's table and is gone).
template <class Op, class TB>
__global__ __launch_bounds__(kResThreads) void mg_restrict_block_kernel(typename Op::Level A, int t0, int t1, int t2,
                                                                        int g0n, int g1n, int k,
                                                                        const typename Op::Scalar *__restrict__ x, long ldx,
                                                                        const TB *__restrict__ b, long ldb,
                                                                        typename Op::Scalar *__restrict__ bc, long ldc,
                                                                        const int *__restrict__ frozen) {
  using S = typename Op::Scalar;
  __shared__ S r[kResLds];
  const int c = blockIdx.y;
  if (!mg_live<1>(c, k, frozen)) return;  // uniform: before any barrier
  const Op op(A);
  const MgLevelArgT<S> &L = op.geo();
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
      const S *__restrict__ xc = x + (size_t)c * ldx;
      auto X = [&](long j, S) { return xc[j]; };
      r[t] = (S)b[(size_t)c * ldb + i] - op.ax_row(row, X, i, g0, g1, g2);
    } else {
      r[t] = 0;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < t0 * t1 * t2) {
    const int j0 = t % t0, q = t / t0, j1 = q % t1, j2 = q / t1;
    if (J0 + j0 < L.nc[0] && J1 + j1 < L.nc[1] && J2 + j2 < L.nc[2]) {
      const long jc = (J0 + j0) + (long)L.nc[0] * ((J1 + j1) + (long)L.nc[1] * (J2 + j2));
      auto at = [&](int a0, int a1, int a2) { return r[a0 + F0 * (a1 + F1 * a2)]; };
      bc[(size_t)c * ldc + jc] = mg_restrict_point(L, at, j0, j1, j2);
    }
  }
}

// x += P e: one index split per point, then the columns
template <int KC, class S>
__global__ __launch_bounds__(256) void mg_prolong_block_kernel(MgLevelArgT<S> L, long N, int k, const S *__restrict__ e,
                                                               long lde, S *__restrict__ x, long ldx,
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
    const S *__restrict__ ec = e + (size_t)(c0 + c) * lde;
    S *__restrict__ xc = x + (size_t)(c0 + c) * ldx;
    auto E = [&](long j) { return ec[j]; };
    xc[i] = xc[i] + mg_prolong_point(L, E, i0, i1, i2);
  }
}

// ------------------------------------------------------------------ the tail: one workgroup, vectors in LDS

// one sweep of a level in LDS: every thread forms its points' new values, then all are written
template <class Op>
__device__ __forceinline__ void tail_sweep(const Op &op, int N, typename Op::Scalar *xs, const typename Op::Scalar *bs) {
  using S = typename Op::Scalar;
  auto X = [&](long k) { return xs[k]; };
  S xn[kTailPts];
#pragma unroll
  for (int p = 0; p < kTailPts; ++p) {
    const int i = threadIdx.x + p * kTailThreads;
    xn[p] = 0;
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
// so do its coefficient arrays: 14 kTailT doubles for the top tail level alone do not fit LDS).  TB / TX: the elements of
// the tail's input and output -- the caller's doubles when the whole grid is the tail, else the level's S.
template <class Op, class TB, class TX>
__device__ __forceinline__ void mg_tail_body(const TailArg<typename Op::Level> *__restrict__ T,
                                             const typename Op::Scalar *__restrict__ minv, const TB *__restrict__ bin,
                                             TX *__restrict__ xout) {
  using S = typename Op::Scalar;
  using Geo = MgLevelArgT<S>;
  __shared__ S sh[kTailLds];
  S *const scr = sh + 4 * kTailT;
  S *const mi = sh + 5 * kTailT;
  const int nl = T->nlev, steps = T->steps, tid = threadIdx.x;
  {
    const Geo &L = level_geo(T->lev[0]);
    const int N = L.n[0] * L.n[1] * L.n[2];
    S *bs = sh + 2 * kTailT + T->off[0];
    for (int i = tid; i < N; i += kTailThreads) bs[i] = (S)bin[i];
    const Geo &C = level_geo(T->lev[nl - 1]);
    const int nc = C.n[0] * C.n[1] * C.n[2];
    for (int i = tid; i < nc * nc; i += kTailThreads) mi[i] = minv[i];
  }
  __syncthreads();
  // down
  for (int l = 0; l < nl - 1; ++l) {
    const Op op(T->lev[l]);
    const Geo &L = op.geo();
    const int N = L.n[0] * L.n[1] * L.n[2], Nc = L.nc[0] * L.nc[1] * L.nc[2];
    S *xs = sh + T->off[l], *bs = sh + 2 * kTailT + T->off[l], *bn = sh + 2 * kTailT + T->off[l + 1];
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
      return (a0 < L.n[0] && a1 < L.n[1] && a2 < L.n[2]) ? scr[a0 + L.n[0] * (a1 + L.n[1] * a2)] : S(0);
    };
    for (int j = tid; j < Nc; j += kTailThreads) {
      const int j0 = j % L.nc[0], q = j / L.nc[0], j1 = q % L.nc[1], j2 = q / L.nc[1];
      bn[j] = mg_restrict_point(L, at, j0, j1, j2);
    }
    __syncthreads();
  }
  // the coarsest level: x = A^-1 b with the inverse formed at creation
  {
    const Geo &C = level_geo(T->lev[nl - 1]);
    const int nc = C.n[0] * C.n[1] * C.n[2];
    S *xs = sh + T->off[nl - 1];
    const S *bs = sh + 2 * kTailT + T->off[nl - 1];
    if (tid < nc) {
      S s = 0;
      for (int j = 0; j < nc; ++j) s += mi[tid * nc + j] * bs[j];
      xs[tid] = s;
    }
    __syncthreads();
  }
  // up
  for (int l = nl - 2; l >= 0; --l) {
    const Op op(T->lev[l]);
    const Geo &L = op.geo();
    const int N = L.n[0] * L.n[1] * L.n[2];
    S *xs = sh + T->off[l];
    const S *bs = sh + 2 * kTailT + T->off[l], *en = sh + T->off[l + 1];
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
    const Geo &L = level_geo(T->lev[0]);
    const int N = L.n[0] * L.n[1] * L.n[2];
    const S *xs = sh + T->off[0];
    for (int i = tid; i < N; i += kTailThreads) xout[i] = (TX)xs[i];
  }
}

template <class Op, class TB, class TX>
__global__ __launch_bounds__(kTailThreads) void mg_tail_kernel(const TailArg<typename Op::Level> *__restrict__ T,
                                                               const typename Op::Scalar *__restrict__ minv,
                                                               const TB *__restrict__ bin, TX *__restrict__ xout) {
  mg_tail_body<Op>(T, minv, bin, xout);
}

// the block form: workgroup c runs the tail on column c's pointers; a frozen column's workgroup returns at once
template <class Op, class TB, class TX>
__global__ __launch_bounds__(kTailThreads) void mg_tail_block_kernel(const TailArg<typename Op::Level> *__restrict__ T,
                                                                     const typename Op::Scalar *__restrict__ minv,
                                                                     const TB *__restrict__ bin, long ldb,
                                                                     TX *__restrict__ xout, long ldx,
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
#include "psp_mg_line.h"
#include "psp_mg_interp.h"

// ====================================================================== the handle

struct psp_mg {
  int n = 0, ndim = 0, steps = 2;
  double omega = 0.8;
  // precision='single' (section 9g): every vector and array below holds floats, `af` and `glev32` are what the kernels
  // take; `a` (and the geometry in `glev`) stays as formed in double
  bool single = false;
  struct Level {
    MgLevelArg a;
    MgLevelArgT<float> af;
    long N = 0;
  };
  std::vector<Level> lev;
  // a level's vectors (mg_alloc_vectors has the rule for which exist): doubles, or floats on a single-precision handle;
  // cols columns of leading dimension N.  `vec`: the single cycle's, one column, allocated at creation.  `blk`: the block
  // cycle's (section 9e), blk_cols columns, allocated by the first block call and grown on demand.
  struct Vecs {
    DevArray<char> x, b, t;
  };
  std::vector<Vecs> vec, blk;
  int blk_cols = 0;
  size_t blk_bytes = 0;
  int tail_first = 0;  // first level of the tail launch
  int launches = 0;    // kernel launches of one application
  DevArray<char> minv;   // the coarsest level's inverse, in the handle's scalar type
  DevArray<char> tail;   // the mode's TailArg on the device
  // galerkin = True (psp_mg_galerkin.h): the stored level operators; `coef` owns each level's arrays in one allocation
  // (diagonal, omega / diagonal, the lower arrays).  A single-precision handle keeps the rounded arrays in `coef32`; its
  // `coef[l]` lives only until level l + 1 is built and level l is rounded.
  bool galerkin = false;
  std::vector<GLevel> glev;
  std::vector<GLevelT<float>> glev32;
  std::vector<DevArray<double>> coef;
  std::vector<DevArray<float>> coef32;
  size_t op_bytes = 0, vec_bytes = 0;  // what the handle holds at rest (psp_mg_bytes)
  // line = a (psp_mg_line.h; section 9h): the axis that is solved exactly and never coarsened, -1 without.  Per level the
  // geometry of its grid lines and the lower array of offset -st_a; the level's second array holds q, not omega / diagonal.
  // Every level is launches: `tail_first` is the last level, which the schedule's tail step solves as the one line it is.
  int line_axis = -1;
  std::vector<MgLine> lines;
  std::vector<const double *> line_lo;
  // stencil='box' (section 9i): level 0 of a stored handle has the full pattern like every level below it
  bool box = false;
  // interp='operator' (psp_mg_interp.h; section 9j): per level above the last the 2^ndim weight arrays of its prolongation
  // in one allocation, and the points of the level that took the linear weights.  No tail launch: `tail_first` is the last
  // level, whose dense product the schedule's tail step launches on its own (`tail` stays null, `minv` is used).
  bool interp = false;
  std::vector<DevArray<double>> wts;
  std::vector<long long> fallbacks;
};

namespace {

// what the kernels of scalar type S take of level l
template <class S>
const MgLevelArgT<S> &mf_level(const psp_mg *K, int l) {
  if constexpr (std::is_same_v<S, double>)
    return K->lev[l].a;
  else
    return K->lev[l].af;
}
template <class S>
const GLevelT<S> &g_level(const psp_mg *K, int l) {
  if constexpr (std::is_same_v<S, double>)
    return K->glev[l];
  else
    return K->glev32[l];
}

// the level's numbers rounded once to float (section 9g); rs is a power of two
MgLevelArgT<float> mg_round_level(const MgLevelArg &a) {
  MgLevelArgT<float> f;
  for (int x = 0; x < 3; ++x) f.n[x] = a.n[x], f.co[x] = a.co[x], f.nc[x] = a.nc[x], f.c[x] = (float)a.c[x];
  f.d = (float)a.d;
  f.w = (float)a.w;
  f.rs = (float)a.rs;
  return f;
}

const char *const kSingleRange =
    "multigrid(precision='single'): a level diagonal or omega / diagonal is outside the single-precision range (not finite, "
    "not > 0 or below FLT_MIN after rounding to float32); precision='double' takes this operator";

template <class S>
int level_nd(const MgLevelArgT<S> &a) {
  return a.n[2] > 1 ? 3 : a.n[1] > 1 ? 2 : 1;
}

// coarse points per workgroup of mg_restrict along each axis (256 in all): by the axes the level really has
template <class S>
void mg_tile(const MgLevelArgT<S> &a, int t[3]) {
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
  DevArray<int> bad_dev;
  PSP_TRY(bad_dev.alloc(1));
  hipError_t e = hipMemsetAsync(bad_dev, 0, sizeof(int), stream());
  if (e == hipSuccess) {
    launch(bad_dev);
    e = hipGetLastError();
  }
  return e == hipSuccess ? read_flag(bad_dev, bad) : fail(PSP_ENODEV, "multigrid: %s", hipGetErrorString(e));
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
int mg_level_grids(psp_mg *K, const int n[3], int steps, int line = -1, bool notail = false) {
  int cur[3] = {n[0], n[1], n[2]};
  for (;;) {
    psp_mg::Level L;
    memset(&L.a, 0, sizeof L.a);
    memset(&L.af, 0, sizeof L.af);
    int coarsened = 0;
    for (int a = 0; a < 3; ++a) {
      L.a.n[a] = cur[a];
      L.a.co[a] = line < 0 ? cur[a] >= 4 : (a != line && cur[a] >= 2);  // section 9h: 3 -> 1 and 2 -> 1 included
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
  if (line >= 0) {
    // no tail kernel: per level above the last `steps` sweeps, the restriction, the prolongation and `steps` sweeps; one
    // solve of the last level, which is a single line
    K->launches = (nl - 1) * (2 * steps + 2) + 1;
    if (nl > kMaxLevels) return fail(PSP_EINVAL, "multigrid: too many levels");
    return PSP_OK;
  }
  if (notail) {
    // section 9j: the launches of every level above the last as below, and the dense product of the last one
    K->launches = (nl - 1) * ((steps >= 2 ? steps - 1 : 1) + 1 + 1 + steps) + 1;
    if (nl > kMaxLevels) return fail(PSP_EINVAL, "multigrid: too many levels");
    return PSP_OK;
  }
  while (K->tail_first > 0 && K->lev[K->tail_first - 1].N <= kTailT) --K->tail_first;
  // launches of one application: per large level the pre-smoothing (the first two sweeps are one pass), the restriction,
  // the prolongation and the post-smoothing; one for the tail
  K->launches = 1;
  for (int l = 0; l < K->tail_first; ++l) K->launches += (steps >= 2 ? steps - 1 : 1) + 1 + 1 + steps;
  if (nl - K->tail_first > kTailMaxLev || nl > kMaxLevels) return fail(PSP_EINVAL, "multigrid: too many levels");
  return PSP_OK;
}

// The level vectors of the handle, `cols` columns wide, into *set; *total grows by the bytes allocated.  The finest level
// works in the caller's vectors and one spare; a level that heads the tail needs its b and x in memory (the restriction
// above it writes b, the prolongation reads x); the levels inside the tail have none.  A single-precision handle holds
// floats, and an x of its own for the finest level too when that level is not the tail: the caller's y is double and takes
// only the last sweep (mg_schedule).  false: an allocation failed; what was allocated is in *set for the caller to drop.
bool mg_alloc_vectors(const psp_mg *K, int cols, std::vector<psp_mg::Vecs> *set, size_t *total) {
  *set = std::vector<psp_mg::Vecs>(K->lev.size());
  for (int l = 0; l <= K->tail_first; ++l) {
    psp_mg::Vecs &V = (*set)[l];
    const size_t bytes = (K->single ? sizeof(float) : sizeof(double)) * (size_t)K->lev[l].N * (size_t)cols;
    const bool own_x = l > 0 || (K->single && K->tail_first > 0);
    DevArray<char> *const want[3] = {l < K->tail_first ? &V.t : nullptr, own_x ? &V.x : nullptr, l > 0 ? &V.b : nullptr};
    for (DevArray<char> *p : want) {
      if (!p) continue;
      if (!p->try_alloc(bytes)) return false;
      *total += bytes;
    }
  }
  return true;
}
// the single cycle's set, at creation (the handle is destroyed when this fails)
int mg_alloc_own_vectors(psp_mg *K) {
  if (!mg_alloc_vectors(K, 1, &K->vec, &K->vec_bytes)) return fail(PSP_ENOMEM, "multigrid: level vector allocation failed");
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
  // the inverse was formed in double; a single-precision handle keeps it rounded to float
  const std::vector<float> inv32(K->single ? inv.begin() : inv.end(), inv.end());
  const void *src = K->single ? (const void *)inv32.data() : (const void *)inv.data();
  const size_t bytes = (K->single ? sizeof(float) : sizeof(double)) * inv.size();
  if (!K->minv.try_alloc(bytes) || !K->tail.try_alloc(sizeof T) ||
      hipMemcpy(K->minv, src, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(K->tail, &T, sizeof T, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PSP_ENOMEM, "multigrid: tail table allocation failed");
  }
  K->op_bytes += bytes + sizeof T;
  return PSP_OK;
}

// interp='operator' (section 9j): the coarsest level's inverse alone -- there is no tail launch and no table of it
int mg_upload_inverse(psp_mg *K, const std::vector<double> &inv) {
  const size_t bytes = sizeof(double) * inv.size();
  if (!K->minv.try_alloc(bytes) || hipMemcpy(K->minv, inv.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PSP_ENOMEM, "multigrid: coarsest inverse allocation failed");
  }
  K->op_bytes += bytes;
  return PSP_OK;
}

// the handle of either mode: build(K) is everything that can fail once it exists (it is destroyed then)
template <class Build>
int mg_make(const psp_csr *A, int ndim, double omega, int steps, bool galerkin, bool single, psp_mg **out,
            Build &&build) {
  psp_mg *K = new psp_mg();
  K->single = single;
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

int mg_create(psp_csr *A, int ndim, const int *grid, double omega, int steps, bool single, psp_mg **out) {
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

  return mg_make(A, ndim, omega, steps, false, single, out, [&](psp_mg *K) {
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
      if (single) {
        L.af = mg_round_level(L.a);
        if (!(L.af.d >= FLT_MIN && L.af.d <= FLT_MAX) || !(L.af.w >= FLT_MIN && L.af.w <= FLT_MAX))
          return fail(PSP_EINVAL, "%s", kSingleRange);
      }
    }
    PSP_TRY(mg_alloc_own_vectors(K));
    std::vector<double> inv;
    PSP_TRY(coarsest_inverse(K->lev.back().a, &inv));
    if (single) return mg_upload_tail(K, inv, [&](int l) { return K->lev[l].af; });
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

// the same for a box handle (section 9i), whose pass knows the kinds offset, duplicate, diagonal and symmetry
const char *g_why_box(int bits) {
  if (bits & kGBadOffset) return "an entry at an offset outside the box: a column more than one point away along an axis of the grid";
  if (bits & kGBadDup) return "an entry that is stored twice";
  if (bits & kGBadDiag) return "a diagonal entry that is missing, or not finite and > 0";
  return "an unsymmetric pair, A[r, c] != A[c, r]";
}

GOut g_out(const GLevel &G) {
  GOut o;
  o.diag = const_cast<double *>(G.diag);
  o.w = const_cast<double *>(G.w);
  for (int k = 0; k < kGMaxOff; ++k) o.lo[k] = const_cast<double *>(G.lo[k]);
  return o;
}

int g_bad_shape(int nd, int noff) {
  return fail(PSP_EINVAL, "multigrid: internal error (a level of %d axes with %d lower arrays)", nd, noff);
}

// f(GShape<ND, NOFF>{}) for the level's shape: the one place that turns (nd, noff) into template arguments
template <int ND, int NOFF>
struct GShape {
  static constexpr int nd = ND, noff = NOFF;
};
template <class S, class F>
int g_dispatch(const GLevelT<S> &G, F &&f) {
  switch (G.nd * 16 + G.noff) {
    case 1 * 16 + 1: f(GShape<1, 1>{}); break;
    case 2 * 16 + 2: f(GShape<2, 2>{}); break;
    case 2 * 16 + 4: f(GShape<2, 4>{}); break;
    case 3 * 16 + 3: f(GShape<3, 3>{}); break;
    case 3 * 16 + 13: f(GShape<3, 13>{}); break;
    default: return g_bad_shape(G.nd, G.noff);
  }
  return PSP_OK;
}

// box: the chain of a box handle (section 9i), whose sums keep their rounding errors; in 1-D the patterns coincide and so do
// the bits
int launch_galerkin(const GLevel &S, long Nc, double omega, const GOut &o, int *flag, bool box) {
  const dim3 grid((unsigned)((Nc + 255) / 256));
  if (box && S.nd == 2 && S.noff == g_full_noff(2)) {
    hipLaunchKernelGGL(mg_galerkin_box_kernel<2>, grid, dim3(256), 0, stream(), S, Nc, omega, o, flag);
    return PSP_OK;
  }
  if (box && S.nd == 3 && S.noff == g_full_noff(3)) {
    hipLaunchKernelGGL(mg_galerkin_box_kernel<3>, grid, dim3(256), 0, stream(), S, Nc, omega, o, flag);
    return PSP_OK;
  }
  return g_dispatch(S, [&](auto sh) {
    hipLaunchKernelGGL((mg_galerkin_kernel<sh.nd, sh.noff>), dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, stream(), S,
                       Nc, omega, o, flag);
  });
}

// interp='operator' (section 9j): the weights of level l's prolongation from its stored stencil -- round m computes the
// points that lie between coarse points along m axes from the rounds before it --, then A_{l+1} = R A_l P with them.
// counter: the level's count of points that took the linear weights, on the device
int launch_weights_galerkin(psp_mg *K, int l, double omega, unsigned long long *counter, int *flag) {
  const GLevel &S = K->glev[l];
  const long N = K->lev[l].N, Nc = K->lev[l + 1].N;
  const size_t bytes = sizeof(double) * ((size_t)N << S.nd);
  if (!K->wts[l].try_alloc((size_t)N << S.nd))
    return fail(PSP_ENOMEM, "multigrid(interp='operator'): weight allocation failed");
  K->op_bytes += bytes;
  double *W = K->wts[l];
  const GOut o = g_out(K->glev[l + 1]);
  return g_dispatch(S, [&](auto sh) {
    for (int round = 0; round <= sh.nd; ++round)
      hipLaunchKernelGGL((mg_weights_kernel<sh.nd, sh.noff>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream(), S, N,
                         round, W, counter);
    hipLaunchKernelGGL((mg_galerkin_w_kernel<sh.nd, sh.noff>), dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, stream(), S,
                       (const double *)W, N, Nc, omega, o, flag);
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

// the arrays of level l in one allocation of scalar type S (diagonal, omega / diagonal, the lower arrays), and the
// level's pointers into it
template <class S>
int g_alloc_level(psp_mg *K, int l, DevArray<S> *owner, GLevelT<S> *G) {
  const size_t N = (size_t)K->lev[l].N;
  if (!owner->try_alloc((size_t)(2 + G->noff) * N)) return fail(PSP_ENOMEM, "multigrid: level operator allocation failed");
  G->diag = *owner;
  G->w = *owner + N;
  for (int k = 0; k < G->noff; ++k) G->lo[k] = *owner + (size_t)(2 + k) * N;
  return PSP_OK;
}

// precision='single': level l's double arrays rounded into float ones (flag: mg_round_kernel's), then released -- the
// next level has been built from them by now.  hipFree waits for the kernels that still read them.
int g_round_level(psp_mg *K, int l, int *flag) {
  const GLevel &G = K->glev[l];
  GLevelT<float> &F = K->glev32[l];
  memset(&F, 0, sizeof F);
  F.a = mg_round_level(G.a);
  F.nd = G.nd;
  F.noff = G.noff;
  memcpy(F.od, G.od, sizeof F.od);
  PSP_TRY(g_alloc_level(K, l, &K->coef32[l], &F));
  const long N = K->lev[l].N, total = (long)(2 + G.noff) * N;
  hipLaunchKernelGGL(mg_round_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream(), total, 2 * N,
                     (const double *)K->coef[l], K->coef32[l], flag);
  PSP_LAUNCH_CHECK();
  K->op_bytes += sizeof(float) * (size_t)total;
  return PSP_OK;
}
void g_release_double(psp_mg *K, int l) {
  K->coef[l].reset();
  GLevel &G = K->glev[l];
  G.diag = G.w = nullptr;
  for (int k = 0; k < kGMaxOff; ++k) G.lo[k] = nullptr;
}

// line = a (section 9h): the grid lines of every level and the factorisation of its line operator, q over omega / diagonal
// (which nothing of this mode reads); *flag is the Galerkin chain's, where the factorisation adds bit 1
int g_build_lines(psp_mg *K, int *flag) {
  const int nl = (int)K->lev.size(), a = K->line_axis, au = a == 0 ? 1 : 0, av = a == 2 ? 1 : 2;
  K->lines.resize(nl);
  K->line_lo.resize(nl);
  for (int l = 0; l < nl; ++l) {
    const GLevel &G = K->glev[l];
    const long st[3] = {1, G.a.n[0], (long)G.a.n[0] * G.a.n[1]};
    MgLine &g = K->lines[l];
    g.n = G.a.n[a], g.nu = G.a.n[au], g.nv = G.a.n[av];
    g.a = a, g.au = au, g.av = av;
    g.st = st[a], g.su = st[au], g.sv = st[av];
    const int slot = g_slot(G.nd, G.noff, a == 0 ? -1 : 0, a == 1 ? -1 : 0, a == 2 ? -1 : 0);
    if (slot < 0) return g_bad_shape(G.nd, G.noff);
    K->line_lo[l] = G.lo[slot];
    const long lines = (long)g.nu * g.nv;
    hipLaunchKernelGGL(mg_line_factor_kernel, dim3((unsigned)((lines + kLineThreads - 1) / kLineThreads)), dim3(kLineThreads), 0,
                       stream(), g, G.diag, K->line_lo[l], const_cast<double *>(G.w), flag);
    PSP_LAUNCH_CHECK();
  }
  int bad = 0;
  PSP_TRY(read_flag(flag, &bad));
  if (bad & 1) return fail(PSP_ESINGULAR, "multigrid(galerkin=True): a level operator's diagonal is not finite and > 0");
  if (bad & 2)
    return fail(PSP_ESINGULAR, "multigrid(line=%d): a pivot of a level's line operator is not finite and > 0 (the matrix is not "
                "positive definite along the lines of axis %d)", a, a);
  return PSP_OK;
}

// mg_create_galerkin's part of mg_make; flags: three ints on the device (the extraction's, the Galerkin product's, the
// rounding's); counters: with interp='operator' one zeroed counter per level on the device, else null
int g_build(psp_mg *K, const psp_csr *A, const int n[3], int *flags, unsigned long long *counters = nullptr) {
  const double omega = K->omega;
  const bool single = K->single;
  const int nd = n[2] > 1 ? 3 : n[1] > 1 ? 2 : 1;
  PSP_TRY(mg_level_grids(K, n, K->steps, K->line_axis, K->interp));  // section 9c's, or with a line axis section 9h's
  const int nl = (int)K->lev.size();
  if (K->interp) {
    K->wts.resize(nl);
    K->fallbacks.assign(nl, 0);
  }
  // the level vectors and the level operators' arrays (a single-precision handle allocates a level's double arrays only
  // when it builds the level)
  PSP_TRY(mg_alloc_own_vectors(K));
  K->glev.resize(nl);
  K->coef.resize(nl);
  if (single) {
    K->glev32.resize(nl);
    K->coef32.resize(nl);
  }
  for (int l = 0; l < nl; ++l) {
    psp_mg::Level &L = K->lev[l];
    GLevel &G = K->glev[l];
    memset(&G, 0, sizeof G);
    G.a = L.a;
    if (single) L.af = mg_round_level(L.a);  // the prolongation's geometry
    G.nd = nd;
    G.noff = l == 0 && !K->box ? nd : g_full_noff(nd);
    for (int k = 0; k < G.noff; ++k)
      for (int a = 0; a < 3; ++a) G.od[k][a] = g_d(nd, G.noff, k, a);
    if (!single || l == 0) {
      PSP_TRY(g_alloc_level(K, l, &K->coef[l], &G));
      if (!single) K->op_bytes += sizeof(double) * (size_t)(2 + G.noff) * (size_t)L.N;
    }
  }
  // level 0: the checking pass writes it
  PSP_HIP(hipMemsetAsync(flags, 0, 3 * sizeof(int), stream()));
  PSP_HIP(hipMemsetAsync(K->coef[0], 0, sizeof(double) * (size_t)(2 + K->glev[0].noff) * (size_t)K->lev[0].N, stream()));
  if (K->box)
    hipLaunchKernelGGL(mg_extract_box_kernel, dim3((A->nrows + 255) / 256), dim3(256), 0, stream(), A->nrows, n[0], n[1], n[2],
                       omega, (const int *)A->ind, (const int *)A->col, (const double *)A->val, g_out(K->glev[0]), flags);
  else
    hipLaunchKernelGGL(mg_extract_csr_kernel, dim3((A->nrows + 255) / 256), dim3(256), 0, stream(), A->nrows, n[0], n[1], n[2],
                       omega, (const int *)A->ind, (const int *)A->col, (const double *)A->val, g_out(K->glev[0]), flags);
  PSP_LAUNCH_CHECK();
  int bad = 0;
  PSP_TRY(read_flag(flags, &bad));
  if (bad && K->box)
    return fail(PSP_EINVAL, "multigrid(galerkin=True, stencil='box'): the matrix is not a symmetric 9- / 27-point stencil on this grid: it has %s",
                g_why_box(bad));
  if (bad)
    return fail(PSP_EINVAL, "multigrid(galerkin=True): the matrix is not a symmetric 3- / 5- / 7-point stencil on this grid: it has %s",
                g_why(bad));
  // A_{l+1} = R_l A_l P_l, level by level
  for (int l = 0; l + 1 < nl; ++l) {
    if (single) PSP_TRY(g_alloc_level(K, l + 1, &K->coef[l + 1], &K->glev[l + 1]));
    if (K->interp)
      PSP_TRY(launch_weights_galerkin(K, l, omega, counters + l, flags + 1));
    else
      PSP_TRY(launch_galerkin(K->glev[l], K->lev[l + 1].N, omega, g_out(K->glev[l + 1]), flags + 1, K->box));
    PSP_LAUNCH_CHECK();
    if (single) {
      PSP_TRY(g_round_level(K, l, flags + 2));
      g_release_double(K, l);
    }
  }
  if (K->line_axis >= 0) return g_build_lines(K, flags + 1);
  // the coarsest level: downloaded and inverted on the host (in double in either precision)
  const GLevel &C = K->glev[nl - 1];
  const int m = (int)K->lev[nl - 1].N;
  std::vector<double> blk((size_t)(2 + C.noff) * m), M, inv;
  PSP_HIP(hipMemcpyAsync(blk.data(), K->coef[nl - 1], sizeof(double) * blk.size(), hipMemcpyDeviceToHost, stream()));
  if (single) PSP_TRY(g_round_level(K, nl - 1, flags + 2));
  // the two flags of the chain, read once
  int chain[2] = {0, 0};
  PSP_HIP(hipMemcpyAsync(chain, flags + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, stream()));
  if (K->interp)
    PSP_HIP(hipMemcpyAsync(K->fallbacks.data(), counters, nl * sizeof(long long), hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  if (single) g_release_double(K, nl - 1);
  if (chain[0]) return fail(PSP_ESINGULAR, "multigrid(galerkin=True): a level operator's diagonal is not finite and > 0");
  if (chain[1]) return fail(PSP_EINVAL, "%s", kSingleRange);
  g_dense(C, blk, &M);
  PSP_TRY(dense_inverse(m, M, &inv));
  if (K->interp) return mg_upload_inverse(K, inv);
  if (single) return mg_upload_tail(K, inv, [&](int l) { return K->glev32[l]; });
  return mg_upload_tail(K, inv, [&](int l) { return K->glev[l]; });
}

// line: -1, or the axis of the line smoother (section 9h), which has no single-precision form; box: level 0 in the full
// layout (section 9i), which has no line-smoothed form
int mg_create_galerkin_line(psp_csr *A, int ndim, const int *grid, double omega, int steps, bool single, int line,
                            psp_mg **out, bool box = false, bool interp = false) {
  int n[3];
  PSP_TRY(mg_check_args(A, ndim, grid, omega, steps, out, n));
  if (interp && (line != -1 || single))
    return fail(PSP_EINVAL, "multigrid(interp='operator'): operator-dependent interpolation with %s is not supported",
                line != -1 ? "a line smoother" : "precision='single'");
  if (line != -1 && box) return fail(PSP_EINVAL, "multigrid(line=%d): stencil='box' with a line smoother is not supported", line);
  if (line != -1) {
    if (ndim < 2) return fail(PSP_EINVAL, "multigrid(line=%d): a grid of one axis has no axis left to coarsen", line);
    if (line < 0 || line >= ndim) return fail(PSP_EINVAL, "multigrid(line=%d): the grid has the axes 0 .. %d", line, ndim - 1);
    if (n[line] < 2) return fail(PSP_EINVAL, "multigrid(line=%d): the line axis has %d point, at least 2 are needed", line, n[line]);
    if (single) return fail(PSP_EINVAL, "multigrid(line=%d): the line smoother has no single-precision form", line);
  }
  if (!(A->ind && A->col && A->val) || A->w4_only)
    return fail(PSP_EINVAL, "multigrid(galerkin=True): the handle no longer holds its index arrays on the device");
  PSP_TRY(ensure_device());
  DevArray<int> flags;
  PSP_TRY(flags.alloc(3));
  DevArray<unsigned long long> counters;  // interp='operator': the fallback points of every level
  if (interp && (!counters.try_alloc(kMaxLevels) ||
                 hipMemsetAsync(counters, 0, kMaxLevels * sizeof(unsigned long long), stream()) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(PSP_ENOMEM, "multigrid(interp='operator'): counter allocation failed");
  }
  return mg_make(A, ndim, omega, steps, true, single, out, [&](psp_mg *K) {
    K->line_axis = line;
    K->box = box;
    K->interp = interp;
    return g_build(K, A, n, flags, counters);
  });
}

int mg_create_galerkin(psp_csr *A, int ndim, const int *grid, double omega, int steps, bool single, bool box, psp_mg **out,
                       bool interp = false) {
  return mg_create_galerkin_line(A, ndim, grid, omega, steps, single, -1, out, box, interp);
}

// the flags of psp_mg_create_*_ex: known bits only, and PSP_MG_BOX selects the pattern of a stored level 0
int mg_check_flags(const char *fn, unsigned flags) {
  if (flags & ~(unsigned)(PSP_MG_GALERKIN | PSP_MG_SINGLE | PSP_MG_BOX | PSP_MG_INTERP))
    return fail(PSP_EINVAL, "%s: unknown flags 0x%x", fn, flags);
  if ((flags & PSP_MG_INTERP) && !(flags & PSP_MG_GALERKIN))
    return fail(PSP_EINVAL, "%s: PSP_MG_INTERP (interp='operator') needs PSP_MG_GALERKIN (galerkin=True): the weights come from stored level operators", fn);
  if ((flags & PSP_MG_INTERP) && (flags & PSP_MG_SINGLE))
    return fail(PSP_EINVAL, "%s: PSP_MG_INTERP (interp='operator') with PSP_MG_SINGLE (precision='single') is not supported", fn);
  if ((flags & PSP_MG_BOX) && !(flags & PSP_MG_GALERKIN))
    return fail(PSP_EINVAL, "%s: PSP_MG_BOX (stencil='box') needs PSP_MG_GALERKIN (galerkin=True): the matrix-free mode stores no level 0", fn);
  return PSP_OK;
}

// A vector of the cycle: the handle's scalar type, or (wide) the caller's doubles, which only the finest level of a
// single-precision handle mixes with its own floats.  ld: the leading dimension of a block of columns (column c at
// p + c * ld), 0 for one vector.
struct MVec {
  void *p = nullptr;
  long ld = 0;
  bool wide = true;
  template <class T>
  T *as() const {
    return static_cast<T *>(p);
  }
  bool operator==(const MVec &o) const { return p == o.p; }
  bool operator!=(const MVec &o) const { return p != o.p; }
};

// f(b's element type *, the written vector's element type *): with S = double both are double -- the kernels of a double
// handle exist in that one form; with S = float a wide b is the caller's (float vectors otherwise), and only next to a
// wide b can the written vector be the caller's y.  FINEST = false: the level is not the finest one (a stored level with
// the full pattern below level 0), so the forms with wide vectors are not chosen for it; level 0 of a box handle
// (section 9i) has that pattern too and takes them.
template <class S, bool FINEST = true, class F>
void mg_with_io(const MVec &b, const MVec &out, F &&f) {
  if constexpr (std::is_same_v<S, double>) {
    f(b.as<const double>(), out.as<double>());
  } else if constexpr (!FINEST) {
    f(b.as<const float>(), out.as<float>());
  } else if (!b.wide) {
    f(b.as<const float>(), out.as<float>());
  } else if (!out.wide) {
    f(b.as<const double>(), out.as<float>());
  } else {
    f(b.as<const double>(), out.as<double>());
  }
}
template <class S, bool FINEST = true, class F>
void mg_with_b(const MVec &b, F &&f) {
  if constexpr (std::is_same_v<S, double>)
    f(b.as<const double>());
  else if constexpr (!FINEST)
    f(b.as<const float>());
  else if (b.wide)
    f(b.as<const double>());
  else
    f(b.as<const float>());
}

template <class S>
void mg_restrict_grid(const MgLevelArgT<S> &a, int tile[3], long g[3]) {
  mg_tile(a, tile);
  // at most ceil(nc0 / t0) ceil(nc1 / t1) ceil(nc2 / t2) <= 2^31 / 256 + a few tiles: fits gridDim.x
  for (int x = 0; x < 3; ++x) g[x] = (a.nc[x] + tile[x] - 1) / tile[x];
}

// Columns per thread of the block kernels, by measurement (DESIGN.md section 9e has the register table and the figures).
// The sweep, scale and prolongation kernels take groups of four columns with stored level operators, whose row of up to 27
// coefficients is then loaded once for four columns, and of two in the matrix-free mode, which has nothing to share
// but the index split (two where k <= 2 in both).  The restriction and the tail take one column per workgroup.
constexpr int kBlockKCGalerkin = 4;
constexpr int kBlockKCMatrixFree = 2;
// op_apply_block and psp_pcg_batch run the block cycle in these modes (section 9e's routing decision)
constexpr bool kRouteBlockMatrixFree = true;
constexpr bool kRouteBlockGalerkin = true;

template <class Op>
struct OpTag {
  using type = Op;
};
template <int KC>
struct KCols {
  static constexpr int kc = KC;
};
template <class P>
using Elem = std::remove_const_t<std::remove_pointer_t<P>>;

// What the steps of the schedule below launch: the first pass from x = 0 (x = w b when steps = 1, else sweeps one and two
// in one pass over b), a further sweep, b_c = R (b - A x), the tail, x += P e -- the cycle kernels with the mode's policy,
// in the handle's scalar type S.  For one vector (k = 0: the single kernels on the handle's own level vectors) or a block
// of k columns (the block kernels on K->blk, groups of kc columns in gridDim.y, the frozen flags as the kernels take
// them).  The mode, the level's shape and the element types are decided once each (with_op, mg_with_io / mg_with_b); only
// the innermost launch statement knows whether there are columns.
template <class S>
struct CycleOps {
  psp_mg *K;
  const std::vector<psp_mg::Vecs> &set;
  int k = 0;
  const int *frozen = nullptr;
  int kc = 0;
  using Vec = MVec;
  explicit CycleOps(psp_mg *K_) : K(K_), set(K_->vec) {}
  CycleOps(psp_mg *K_, int k_, const int *frozen_) : K(K_), set(K_->blk), k(k_), frozen(frozen_) {
    kc = k <= 2 ? 2 : K->galerkin ? kBlockKCGalerkin : kBlockKCMatrixFree;
    const char *e = k <= 2 ? nullptr : tuning_env("PSP_MG_BLOCK_KC");  // 2 or 4: the group size that is not the default
    if (e && (atoi(e) == 2 || atoi(e) == 4)) kc = atoi(e);
  }
  Vec vec(void *p, int l) const { return MVec{p, k ? K->lev[l].N : 0, std::is_same_v<S, double>}; }
  Vec lx(int l) const { return vec(set[l].x, l); }
  Vec lb(int l) const { return vec(set[l].b, l); }
  Vec lt(int l) const { return vec(set[l].t, l); }
  // one thread per point; a block's column groups in gridDim.y
  dim3 grid(long N) const {
    const unsigned nb = (unsigned)((N + 255) / 256);
    return k ? dim3(nb, (unsigned)((k + kc - 1) / kc)) : dim3(nb);
  }
  template <class F>
  void with_kc(F &&f) const {
    if (kc == 4)
      f(KCols<4>{});
    else
      f(KCols<2>{});
  }
  // f(OpTag<the policy of level l>, what its kernels take of the level).  SPLIT = false: a matrix-free level of any shape
  // goes through MfOp<3> (the restriction, whose shapes are run-time)
  template <bool SPLIT, class F>
  int with_op(int l, F &&f) const {
    if (K->galerkin) {
      const GLevelT<S> &G = g_level<S>(K, l);
      return g_dispatch(G, [&](auto sh) { f(OpTag<GOp<sh.nd, sh.noff, S>>{}, G); });
    }
    const MgLevelArgT<S> &a = mf_level<S>(K, l);
    const int nd = SPLIT ? level_nd(a) : 3;
    if constexpr (SPLIT) {
      if (nd == 1) f(OpTag<MfOp<1, S>>{}, a);
      if (nd == 2) f(OpTag<MfOp<2, S>>{}, a);
    }
    if (nd == 3) f(OpTag<MfOp<3, S>>{}, a);
    return PSP_OK;
  }

  template <bool FROMB>
  int smooth(int l, Vec xin, Vec b, Vec xout) const {
    const long N = K->lev[l].N;
    return with_op<true>(l, [&](auto tag, const auto &A) {
      using Op = typename decltype(tag)::type;
      auto launch = [&](auto *bp, auto *op) {
        using TB = Elem<decltype(bp)>;
        using TO = Elem<decltype(op)>;
        if (!k)
          hipLaunchKernelGGL((mg_smooth_kernel<Op, FROMB, TB, TO>), grid(N), dim3(256), 0, stream(), A, N, xin.as<const S>(), bp,
                             op);
        else
          with_kc([&](auto c) {
            hipLaunchKernelGGL((mg_smooth_block_kernel<Op, FROMB, c.kc, TB, TO>), grid(N), dim3(256), 0, stream(), A, N, k,
                               xin.as<const S>(), xin.ld, bp, b.ld, op, xout.ld, frozen);
          });
      };
      // level 0 of a box handle (section 9i) has the full pattern and is the finest level all the same
      if (l == 0)
        mg_with_io<S, true>(b, xout, launch);
      else
        mg_with_io<S, Op::kFinest>(b, xout, launch);
    });
  }
  // line = a (section 9h): one line sweep of level l, xout = xin + omega T^-1 (b - A xin); FROM0: from xin = 0.  The line
  // kernels have no block form: mg_apply_block_dev sends a line handle's columns through here one at a time
  template <bool FROM0>
  int line_sweep(int l, double omega, Vec xin, Vec b, Vec xout) const {
    if constexpr (std::is_same_v<S, double>) {
      const GLevel &G = K->glev[l];
      const MgLine &g = K->lines[l];
      const long lines = (long)g.nu * g.nv;
      return g_dispatch(G, [&](auto sh) {
        hipLaunchKernelGGL((mg_line_sweep_kernel<GOp<sh.nd, sh.noff, double>, FROM0>),
                           dim3((unsigned)((lines + kLineThreads - 1) / kLineThreads)), dim3(kLineThreads), 0, stream(), G, g,
                           omega, K->line_lo[l], xin.as<const double>(), b.as<const double>(), xout.as<double>());
      });
    } else {
      return fail(PSP_EINVAL, "multigrid: internal error (a single-precision handle with a line axis)");
    }
  }
  template <class W>  // MfW or GW
  void scale(int l, W w, Vec b, Vec dst) const {
    const long N = K->lev[l].N;
    mg_with_b<S>(b, [&](auto *bp) {
      using TB = Elem<decltype(bp)>;
      if (!k)
        hipLaunchKernelGGL((mg_scale_kernel<W, TB>), grid(N), dim3(256), 0, stream(), N, w, bp, dst.as<S>());
      else
        with_kc([&](auto c) {
          hipLaunchKernelGGL((mg_scale_block_kernel<W, c.kc, TB>), grid(N), dim3(256), 0, stream(), N, w, k, bp, b.ld,
                             dst.as<S>(), dst.ld, frozen);
        });
    });
  }
  int first(int l, Vec b, Vec dst) const {
    if (K->line_axis >= 0) return line_sweep<true>(l, K->omega, Vec(), b, dst);
    if (K->steps > 1) return smooth<true>(l, Vec(), b, dst);
    if (K->galerkin)
      scale(l, GW<S>{g_level<S>(K, l).w}, b, dst);
    else
      scale(l, MfW<S>{mf_level<S>(K, l).w}, b, dst);
    return PSP_OK;
  }
  int sweep(int l, Vec xin, Vec b, Vec xout) const {
    if (K->line_axis >= 0) return line_sweep<false>(l, K->omega, xin, b, xout);
    return smooth<false>(l, xin, b, xout);
  }
  // a workgroup per tile of coarse points; a block's columns in gridDim.y, one each
  int restrict_to(int l, Vec x, Vec b, Vec bc) const {
    if (K->interp) return restrict_w(l, x, b, bc);
    return with_op<false>(l, [&](auto tag, const auto &A) {
      using Op = typename decltype(tag)::type;
      int tile[3];
      long g[3];
      mg_restrict_grid(level_geo(A), tile, g);
      const unsigned tiles = (unsigned)(g[0] * g[1] * g[2]);
      auto launch = [&](auto *bp) {
        using TB = Elem<decltype(bp)>;
        if (!k)
          hipLaunchKernelGGL((mg_restrict_kernel<Op, TB>), dim3(tiles), dim3(kResThreads), 0, stream(), A, tile[0], tile[1],
                             tile[2], (int)g[0], (int)g[1], x.as<const S>(), bp, bc.as<S>());
        else
          hipLaunchKernelGGL((mg_restrict_block_kernel<Op, TB>), dim3(tiles, (unsigned)k), dim3(kResThreads), 0, stream(), A,
                             tile[0], tile[1], tile[2], (int)g[0], (int)g[1], k, x.as<const S>(), x.ld, bp, b.ld, bc.as<S>(),
                             bc.ld, frozen);
      };
      if (l == 0)  // as in smooth()
        mg_with_b<S, true>(b, launch);
      else
        mg_with_b<S, Op::kFinest>(b, launch);
    });
  }
  // interp='operator' (section 9j): the transfers with the level's weights and the coarsest level's dense product, each one
  // launch on one vector in double -- such a handle has no single-precision form, and mg_apply_block_dev sends its columns
  // through here one at a time
  int not_weighted() const { return fail(PSP_EINVAL, "multigrid: internal error (weighted transfers on a single-precision handle or a block)"); }
  int restrict_w(int l, Vec x, Vec b, Vec bc) const {
    if constexpr (std::is_same_v<S, double>) {
      if (k) return not_weighted();
      const GLevel &G = K->glev[l];
      int tile[3];
      long g[3];
      mg_restrict_grid(G.a, tile, g);
      const unsigned tiles = (unsigned)(g[0] * g[1] * g[2]);
      return g_dispatch(G, [&](auto sh) {
        hipLaunchKernelGGL((mg_restrict_w_kernel<GOp<sh.nd, sh.noff, double>>), dim3(tiles), dim3(kResThreads), 0, stream(), G,
                           tile[0], tile[1], tile[2], (int)g[0], (int)g[1], (const double *)K->wts[l], K->lev[l].N,
                           x.as<const double>(), b.as<const double>(), bc.as<double>());
      });
    } else {
      return not_weighted();
    }
  }
  void prolong_w(int l, Vec e, Vec x) const {
    if constexpr (std::is_same_v<S, double>) {
      const long N = K->lev[l].N;
      hipLaunchKernelGGL(mg_prolong_w_kernel, grid(N), dim3(256), 0, stream(), K->lev[l].a, N, (const double *)K->wts[l],
                         e.as<const double>(), x.as<double>());
    }
  }
  void dense(Vec b, Vec x) const {
    if constexpr (std::is_same_v<S, double>)
      hipLaunchKernelGGL(mg_dense_kernel, dim3(1), dim3(64), 0, stream(), (int)K->lev[K->tail_first].N, (const double *)K->minv.get(),
                         b.as<const double>(), x.as<double>());
  }
  // the tail's ends are both the caller's (the whole grid is the tail) or both the handle's; a block's columns are a
  // workgroup each
  template <class Op>  // MfOp<3> or GTailOp: K->tail is that mode's table
  void launch_tail(Vec b, Vec x) const {
    const auto *T = (const TailArg<typename Op::Level> *)K->tail.get();
    const S *minv = (const S *)K->minv.get();
    mg_with_io<S>(b, x, [&](auto *bp, auto *xp) {
      using TB = Elem<decltype(bp)>;
      using TX = Elem<decltype(xp)>;
      if constexpr (std::is_same_v<TB, TX>) {
        if (!k)
          hipLaunchKernelGGL((mg_tail_kernel<Op, TB, TX>), dim3(1), dim3(kTailThreads), 0, stream(), T, minv, bp, xp);
        else
          hipLaunchKernelGGL((mg_tail_block_kernel<Op, TB, TX>), dim3(k), dim3(kTailThreads), 0, stream(), T, minv, bp, b.ld, xp,
                             x.ld, frozen);
      }
    });
  }
  // with a line axis the step is the last level's x = T^-1 b: that level is one line and A = T there (section 9h)
  void tail(Vec b, Vec x) const {
    if (K->interp)
      dense(b, x);
    else if (K->line_axis >= 0)
      (void)line_sweep<true>(K->tail_first, 1.0, Vec(), b, x);
    else if (K->galerkin)
      launch_tail<GTailOp<S>>(b, x);
    else
      launch_tail<MfOp<3, S>>(b, x);
  }
  void prolong(int l, Vec e, Vec x) const {
    if (K->interp) return prolong_w(l, e, x);
    const long N = K->lev[l].N;
    const MgLevelArgT<S> &a = mf_level<S>(K, l);
    if (!k)
      hipLaunchKernelGGL(mg_prolong_kernel<S>, grid(N), dim3(256), 0, stream(), a, N, e.as<const S>(), x.as<S>());
    else
      with_kc([&](auto c) {
        hipLaunchKernelGGL((mg_prolong_block_kernel<c.kc, S>), grid(N), dim3(256), 0, stream(), a, N, k, e.as<const S>(), e.ld,
                           x.as<S>(), x.ld, frozen);
      });
  }
};

// the sss entry points: an sss_mat is read through its full device mirror
template <class Create>  // create(the mirror)
int mg_create_sss(psp_sss_t *A, const char *fn, Create &&create) {
  PSP_API_GUARD_H(A, A ? A->full : nullptr);
  if (!A) return fail(PSP_EINVAL, "%s: NULL argument", fn);
  if (A->host || cpu_mode())
    return fail(PSP_ENODEV, "precon.multigrid: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  if (!A->full) return fail(PSP_EINVAL, "%s: the matrix has no device mirror", fn);
  return create(A->full);
}

// one V-cycle: the schedule of launches and buffers, the same in both modes, both precisions and for one vector or a block
// of them: K->launches launches whatever the column count is.  b_dev is only read.  A double handle's finest level works
// in y and one spare; a single-precision one in two float vectors of its own, and only its last sweep writes y.
template <class Ops>
int mg_schedule(psp_mg *K, typename Ops::Vec b_dev, typename Ops::Vec y_dev, const Ops &ops) {
  using V = typename Ops::Vec;
  const int steps = K->steps, tf = K->tail_first;
  const bool own0 = K->single;
  // where each large level's iterate is after its pre-smoothing; every sweep writes the buffer the previous one did not
  V cur[kMaxLevels] = {};
  // down
  for (int l = 0; l < tf; ++l) {
    const V b = l == 0 ? b_dev : ops.lb(l);
    const V own = l == 0 && !own0 ? y_dev : ops.lx(l);
    // the finest level's last sweep must land in y: its writes are the pre-smoothing launches and `steps` more
    // (a line sweep is a launch of its own each: the first two are not one pass)
    const int pre = K->line_axis >= 0 ? steps : steps >= 2 ? steps - 1 : 1;
    const int writes = pre + steps;
    V dst = (l == 0 && !own0 && (writes & 1) == 0) ? ops.lt(l) : own;
    PSP_TRY(ops.first(l, b, dst));
    for (int k = 1; k < pre; ++k) {
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
    const V own = l == 0 && !own0 ? y_dev : ops.lx(l);
    V x = cur[l];
    ops.prolong(l, cur[l + 1], x);
    for (int k = 0; k < steps; ++k) {
      V nxt = x == own ? ops.lt(l) : own;
      if (l == 0 && own0 && k == steps - 1) nxt = y_dev;
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
  K->blk.clear();
  K->blk_cols = 0;
  K->blk_bytes = 0;
}

// the block cycle's level vectors for at least k columns (k = 0: none)
int mg_block_reserve(psp_mg *K, int k) {
  // a line handle has no block vectors to reserve, nor has one with operator-dependent interpolation
  if (k > 0 && (k <= K->blk_cols || K->line_axis >= 0 || K->interp)) return PSP_OK;
  mg_block_free(K);
  if (k == 0) return PSP_OK;
  if (!mg_alloc_vectors(K, k, &K->blk, &K->blk_bytes)) {
    mg_block_free(K);
    return fail(PSP_ENOMEM, "multigrid: block level vector allocation failed (%d columns)", k);
  }
  K->blk_cols = k;
  return PSP_OK;
}

}  // namespace

namespace psp {

// y = V(0, b) on device vectors; y must not alias b.  The handle is locked by the caller.
int mg_apply_dev(psp_mg *K, const double *b_dev, double *y_dev) {
  const MVec b{const_cast<double *>(b_dev), 0, true}, y{y_dev, 0, true};
  if (K->single) return mg_schedule(K, b, y, CycleOps<float>(K));
  return mg_schedule(K, b, y, CycleOps<double>(K));
}

// Y[:, c] = V(0, X[:, c]) for every column c < k with frozen[c] == 0 (frozen == nullptr: every column), one block cycle:
// the bits of mg_apply_dev on the column, K's launches whatever k is.  Y must not overlap X.  The handle is locked by the
// caller.
int mg_apply_block_dev(psp_mg *K, int k, const double *X, long ldx, double *Y, long ldy, const int *frozen) {
  if (K->line_axis >= 0 || K->interp) {
    // the line kernels have no block form (section 9h), nor have the weighted transfers (section 9j): the single cycle
    // column by column, no block vectors.  The frozen flags live on the device, so a caller that has some goes column by
    // column itself (mg_block_routed is false).
    if (frozen)
      return fail(PSP_EINVAL, "multigrid: internal error (a block cycle with frozen columns on %s)",
                  K->interp ? "a handle with interp='operator'" : "a line handle");
    for (int c = 0; c < k; ++c) PSP_TRY(mg_apply_dev(K, X + (size_t)c * ldx, Y + (size_t)c * ldy));
    return PSP_OK;
  }
  PSP_TRY(mg_block_reserve(K, k));
  const MVec x{const_cast<double *>(X), ldx, true}, y{Y, ldy, true};
  if (K->single) return mg_schedule(K, x, y, CycleOps<float>(K, k, frozen));
  return mg_schedule(K, x, y, CycleOps<double>(K, k, frozen));
}

int mg_launches(const psp_mg *K) { return K->launches; }

// Where op_apply_block and the batched PCG loop run the block cycle and where they keep the column-by-column path: by the
// measurements of DESIGN.md section 9e (profiles/mg_block_timing.json).
bool mg_block_routed(const psp_mg *K) {
  if (K->line_axis >= 0 || K->interp) return false;
  return K->galerkin ? kRouteBlockGalerkin : kRouteBlockMatrixFree;
}

}  // namespace psp

namespace {

// The body of the host entry points `fn`: the caller's vector (k = 0) or its k columns of n to scratch, apply(x, y) on the
// device copies (columns of leading dimension n), y back.  The cycle's own error comes before the copies'.
template <class Apply>
int mg_staged(const char *fn, size_t n, int k, const double *x_host, long ldx, double *y_host, long ldy, Apply &&apply) {
  const size_t nk = n * (size_t)std::max(k, 1), row = sizeof(double) * n;
  auto copy = [&](void *dst, size_t dpitch, const void *src, size_t spitch, hipMemcpyKind kind) {
    return k ? hipMemcpy2DAsync(dst, dpitch, src, spitch, row, k, kind, stream())
             : hipMemcpyAsync(dst, src, row, kind, stream());
  };
  double *x = nullptr, *y = nullptr;
  PSP_TRY(scratch_get(nk, &x));
  int rc = scratch_get(nk, &y);
  if (rc != PSP_OK) {
    scratch_put(x, nk);
    return rc;
  }
  hipError_t e = copy(x, row, x_host, sizeof(double) * ldx, hipMemcpyHostToDevice);
  if (e == hipSuccess) rc = apply(x, y);
  if (e == hipSuccess && rc == PSP_OK) e = copy(y_host, sizeof(double) * ldy, y, row, hipMemcpyDeviceToHost);
  const hipError_t e2 = hipStreamSynchronize(stream());
  scratch_put(x, nk);
  scratch_put(y, nk);
  if (rc != PSP_OK) return rc;
  if (e != hipSuccess || e2 != hipSuccess) return fail(PSP_ENODEV, "%s: %s", fn, hipGetErrorString(e != hipSuccess ? e : e2));
  return PSP_OK;
}

}  // namespace

extern "C" {

int psp_mg_create_csr_ex(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, unsigned flags, psp_mg_t **out) {
  PSP_API_GUARD_H(A);
  PSP_TRY(mg_check_flags("psp_mg_create_csr_ex", flags));
  const bool single = (flags & PSP_MG_SINGLE) != 0, box = (flags & PSP_MG_BOX) != 0, interp = (flags & PSP_MG_INTERP) != 0;
  if (flags & PSP_MG_GALERKIN) return mg_create_galerkin(A, ndim, grid, omega, steps, single, box, out, interp);
  return mg_create(A, ndim, grid, omega, steps, single, out);
}

int psp_mg_create_sss_ex(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, unsigned flags, psp_mg_t **out) {
  PSP_TRY(mg_check_flags("psp_mg_create_sss_ex", flags));
  const bool single = (flags & PSP_MG_SINGLE) != 0, box = (flags & PSP_MG_BOX) != 0, interp = (flags & PSP_MG_INTERP) != 0;
  if (flags & PSP_MG_GALERKIN)
    return mg_create_sss(A, "psp_mg_create_sss_galerkin",
                         [&](psp_csr *F) { return mg_create_galerkin(F, ndim, grid, omega, steps, single, box, out, interp); });
  return mg_create_sss(A, "psp_mg_create_sss", [&](psp_csr *F) { return mg_create(F, ndim, grid, omega, steps, single, out); });
}

// galerkin=True with the line smoother along line_axis (section 9h).  Calls of their own: the flags of psp_mg_create_*_ex
// stay what they are.
int psp_mg_create_csr_line(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, int line_axis, psp_mg_t **out) {
  PSP_API_GUARD_H(A);
  if (line_axis < 0) return fail(PSP_EINVAL, "multigrid(line=%d): the line axis must be one of the grid's axes, 0 .. ndim - 1", line_axis);
  return mg_create_galerkin_line(A, ndim, grid, omega, steps, false, line_axis, out);
}

int psp_mg_create_sss_line(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, int line_axis, psp_mg_t **out) {
  if (line_axis < 0) return fail(PSP_EINVAL, "multigrid(line=%d): the line axis must be one of the grid's axes, 0 .. ndim - 1", line_axis);
  return mg_create_sss(A, "psp_mg_create_sss_line",
                       [&](psp_csr *F) { return mg_create_galerkin_line(F, ndim, grid, omega, steps, false, line_axis, out); });
}

int psp_mg_line_axis(const psp_mg_t *K, int *axis) {
  if (!K || !axis) return fail(PSP_EINVAL, "psp_mg_line_axis: NULL argument");
  *axis = K->line_axis;
  return PSP_OK;
}

int psp_mg_stencil(const psp_mg_t *K, int *box) {
  if (!K || !box) return fail(PSP_EINVAL, "psp_mg_stencil: NULL argument");
  *box = K->box ? 1 : 0;
  return PSP_OK;
}

int psp_mg_interp(const psp_mg_t *K, int *operator_dependent) {
  if (!K || !operator_dependent) return fail(PSP_EINVAL, "psp_mg_interp: NULL argument");
  *operator_dependent = K->interp ? 1 : 0;
  return PSP_OK;
}

int psp_mg_interp_fallbacks(psp_mg_t *K, int level, long long *points) {
  PSP_API_GUARD_H(K);
  if (!K || !points) return fail(PSP_EINVAL, "psp_mg_interp_fallbacks: NULL argument");
  if (!K->interp) return fail(PSP_EINVAL, "psp_mg_interp_fallbacks: the handle has no operator-dependent interpolation (interp='linear')");
  if (level < 0 || level + 1 >= (int)K->lev.size()) return fail(PSP_EINVAL, "psp_mg_interp_fallbacks: no transfer from level %d", level);
  *points = K->fallbacks[level];
  return PSP_OK;
}

int psp_mg_transfer_weights(psp_mg_t *K, int level, int *nslots_inout, double *W_host) {
  PSP_API_GUARD_H(K);
  if (!K || !nslots_inout) return fail(PSP_EINVAL, "psp_mg_transfer_weights: NULL argument");
  if (!K->interp) return fail(PSP_EINVAL, "psp_mg_transfer_weights: the handle stores no weights (interp='linear')");
  if (level < 0 || level + 1 >= (int)K->lev.size()) return fail(PSP_EINVAL, "psp_mg_transfer_weights: no transfer from level %d", level);
  const int cap = *nslots_inout, cnt = 1 << K->glev[level].nd;
  *nslots_inout = cnt;
  if (!W_host) return PSP_OK;
  if (cap < cnt) return fail(PSP_EINVAL, "psp_mg_transfer_weights: room for %d slots, the level has %d", cap, cnt);
  PSP_TRY(ensure_device());
  PSP_HIP(hipMemcpyAsync(W_host, K->wts[level], sizeof(double) * (size_t)cnt * (size_t)K->lev[level].N, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

int psp_mg_create_csr(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return psp_mg_create_csr_ex(A, ndim, grid, omega, steps, 0u, out);
}

int psp_mg_create_sss(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return psp_mg_create_sss_ex(A, ndim, grid, omega, steps, 0u, out);
}

int psp_mg_create_csr_galerkin(psp_csr_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return psp_mg_create_csr_ex(A, ndim, grid, omega, steps, PSP_MG_GALERKIN, out);
}

int psp_mg_create_sss_galerkin(psp_sss_t *A, int ndim, const int *grid, double omega, int steps, psp_mg_t **out) {
  return psp_mg_create_sss_ex(A, ndim, grid, omega, steps, PSP_MG_GALERKIN, out);
}

int psp_mg_precision(const psp_mg_t *K, int *bits) {
  if (!K || !bits) return fail(PSP_EINVAL, "psp_mg_precision: NULL argument");
  *bits = K->single ? 32 : 64;
  return PSP_OK;
}

int psp_mg_bytes(const psp_mg_t *K, long long *operator_bytes, long long *vector_bytes) {
  if (!K) return fail(PSP_EINVAL, "psp_mg_bytes: NULL handle");
  if (operator_bytes) *operator_bytes = (long long)K->op_bytes;
  if (vector_bytes) *vector_bytes = (long long)K->vec_bytes;
  return PSP_OK;
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
  const GLevel &G = K->glev[level];  // a single-precision handle keeps the geometry here, the arrays in glev32
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
    if (K->single) {  // the stored floats, widened
      const GLevelT<float> &F = K->glev32[level];
      std::vector<float> tmp(N * (size_t)cnt);
      PSP_HIP(hipMemcpyAsync(tmp.data(), F.diag, sizeof(float) * N, hipMemcpyDeviceToHost, stream()));
      if (F.noff > 0)
        PSP_HIP(hipMemcpyAsync(tmp.data() + N, F.lo[0], sizeof(float) * N * (size_t)F.noff, hipMemcpyDeviceToHost, stream()));
      PSP_HIP(hipStreamSynchronize(stream()));
      for (size_t i = 0; i < tmp.size(); ++i) values_host[i] = (double)tmp[i];
      return PSP_OK;
    }
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
  delete K;
  return PSP_OK;
}

int psp_mg_info(const psp_mg_t *K, int *levels, int *tail_first_level, int *launches_per_apply, int *dims) {
  if (!K) return fail(PSP_EINVAL, "psp_mg_info: NULL handle");
  if (levels) *levels = (int)K->lev.size();
  // a line handle has no tail launch: its last level is one more ordinary launch
  // nor has a handle with operator-dependent interpolation
  if (tail_first_level) *tail_first_level = K->line_axis >= 0 || K->interp ? (int)K->lev.size() : K->tail_first;
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
  return mg_staged("psp_mg_precon", (size_t)K->n, 0, x_host, K->n, y_host, K->n,
                   [&](const double *x, double *y) { return mg_apply_dev(K, x, y); });
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
  return mg_staged("psp_mg_precon_block", (size_t)K->n, k, X_host, ldx, Y_host, ldy, [&](const double *x, double *y) {
    return mg_apply_block_dev(K, k, x, (long)K->n, y, (long)K->n, nullptr);
  });
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
