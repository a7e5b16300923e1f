// psp_mg_line.h -- the line smoother of precon.multigrid: galerkin=True, line=a (DESIGN.md section 9h is the normative
// text).  Part of psp_mg.hip's translation unit, included after psp_mg_galerkin.h, whose stored levels (GLevel) and
// level-operator policy (GOp) it works on.  What only the line mode has: the geometry of a level's grid lines (MgLine),
// the factorisation of the line operator T_l (mg_line_factor_kernel) and the sweep x <- x + omega T_l^-1 (b - A_l x)
// (mg_line_sweep_kernel).  T_l = the diagonal of A_l and its entries at offset -+st_a, tridiagonal along every grid line
// of axis a.  Restriction, prolongation and the Galerkin product are the stored mode's, with axis a never coarsened.
//
// One thread owns one grid line and walks it twice: forward (residual row, elimination, y parked in the output vector),
// then backward (substitution, x_out = x_in + omega e).  Adjacent lanes own lines adjacent along the fastest axis other
// than a: for a >= 1 that axis is axis 0 and every access of a step is coalesced across the wave; for a = 0 the lanes are
// n0 elements apart.  Only the multiply-subtract chain is serial: what a step loads does not depend on it, so the loads
// of kU steps are issued together, ahead of the chain.  Nothing divides inside a solve, there are no atomics and every
// sum has one fixed order: the same bits from run to run.
namespace {

constexpr int kLineThreads = 64;  // one wave per workgroup: a level's lines spread over as many CUs as there are waves

struct MgLine {
  int n;             // points of a line
  int nu, nv;        // lines side by side along the faster and the slower of the other two axes
  int a, au, av;     // the line axis, those two axes
  long st, su, sv;   // the three strides
};

// the coordinates of the line's first point and what a step along the line adds to them
struct MgLineAt {
  long base;
  int c0, c1, c2, d0, d1, d2;
};
__device__ __forceinline__ MgLineAt mg_line_at(const MgLine &g, long t) {
  const int pu = (int)(t % g.nu), pv = (int)(t / g.nu);
  MgLineAt p;
  p.base = pu * g.su + pv * g.sv;
  p.c0 = (g.au == 0 ? pu : 0) + (g.av == 0 ? pv : 0);
  p.c1 = (g.au == 1 ? pu : 0) + (g.av == 1 ? pv : 0);
  p.c2 = (g.au == 2 ? pu : 0) + (g.av == 2 ? pv : 0);
  p.d0 = g.a == 0, p.d1 = g.a == 1, p.d2 = g.a == 2;
  return p;
}

// p_0 = d_0, p_i = d_i - l_i (l_i q_{i-1}), q_i = 1 / p_i with l_i = A_l[K_i, K_i - st_a] (`la`: the level's lower array
// of that offset); q replaces omega / diagonal in the level's second array.  One thread per line; *flag gets bit 1 when
// a pivot is not finite and > 0.
__global__ __launch_bounds__(kLineThreads) void mg_line_factor_kernel(MgLine g, const double *__restrict__ diag,
                                                                      const double *__restrict__ la,
                                                                      double *__restrict__ q, int *__restrict__ flag) {
  constexpr int kU = 8;
  const long t = (long)blockIdx.x * kLineThreads + threadIdx.x;
  if (t >= (long)g.nu * g.nv) return;
  const long base = mg_line_at(g, t).base;
  double qp = 0.0;
  bool ok = true;
  auto step = [&](int i, double d, double l) {
    const double p = i > 0 ? d - l * (l * qp) : d;
    if (!(p > 0.0) || !(p <= DBL_MAX)) ok = false;
    qp = 1.0 / p;
    q[base + i * g.st] = qp;
  };
  int i = 0;
  for (; i + kU <= g.n; i += kU) {
    double d[kU], l[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) d[u] = diag[base + (i + u) * g.st], l[u] = la[base + (i + u) * g.st];
#pragma unroll
    for (int u = 0; u < kU; ++u) step(i + u, d[u], l[u]);
  }
  for (; i < g.n; ++i) step(i, diag[base + i * g.st], la[base + i * g.st]);
  if (!ok) atomicOr(flag, 2);
}

// One sweep of a level, out of place: xout = xin + omega T^-1 (b - A xin), one thread per grid line.
//   forward   y_0 = r_0, y_i = r_i - (l_i q_{i-1}) y_{i-1}, with r_i the residual row in section 9d's order; y is parked
//             in xout, which no other line reads
//   backward  e_{n-1} = q_{n-1} y_{n-1}, e_i = q_i (y_i - l_{i+1} e_{i+1}); xout = xin + omega e
// FROM0: xin = 0, so r = b and xout = omega e -- the first sweep of a level, and with omega = 1 the last level's
// x = T^-1 b.  xout must not be xin: the residual rows of the neighbouring lines read xin.
template <class Op, bool FROM0>
__global__ __launch_bounds__(kLineThreads) void mg_line_sweep_kernel(typename Op::Level A, MgLine g,
                                                                     typename Op::Scalar omega,
                                                                     const typename Op::Scalar *__restrict__ la,
                                                                     const typename Op::Scalar *__restrict__ xin,
                                                                     const typename Op::Scalar *__restrict__ b,
                                                                     typename Op::Scalar *__restrict__ xout) {
  using S = typename Op::Scalar;
  // steps whose loads are in flight together: a row of the full 3-D pattern is 54 loads, of the others at most 19
  constexpr int kUF = Op::kNoff > 4 ? 2 : 4, kUB = 8;
  const long t = (long)blockIdx.x * kLineThreads + threadIdx.x;
  if (t >= (long)g.nu * g.nv) return;
  const Op op(A);
  const S *__restrict__ q = A.w;
  const MgLineAt p = mg_line_at(g, t);
  const long st = g.st;
  const int n = g.n;
  auto X = [&](long k) -> S { return xin[k]; };
  // the residual row of point i of the line and l_i q_{i-1} (0 at i = 0, where l_0 = 0 is stored)
  auto row = [&](int i, S &r, S &m) {
    const long k = p.base + i * st;
    r = b[k];
    if constexpr (!FROM0) r = r - op.ax(X, k, p.c0 + i * p.d0, p.c1 + i * p.d1, p.c2 + i * p.d2);
    m = i > 0 ? la[k] * q[k - st] : S(0);
  };
  S y = 0;
  auto fwd = [&](int i, S r, S m) {
    y = i > 0 ? r - m * y : r;
    xout[p.base + i * st] = y;
  };
  int i = 0;
  for (; i + kUF <= n; i += kUF) {
    S r[kUF], m[kUF];
#pragma unroll
    for (int u = 0; u < kUF; ++u) row(i + u, r[u], m[u]);
#pragma unroll
    for (int u = 0; u < kUF; ++u) fwd(i + u, r[u], m[u]);
  }
  for (; i < n; ++i) {
    S r, m;
    row(i, r, m);
    fwd(i, r, m);
  }
  // backward: point i needs y_i (its own write above), q_i, l_{i+1} and xin_i
  S e = 0;
  auto back = [&](int j, S yj, S qj, S ln, S xj) {
    e = j < n - 1 ? qj * (yj - ln * e) : qj * yj;
    if constexpr (FROM0)
      xout[p.base + j * st] = omega * e;
    else
      xout[p.base + j * st] = xj + omega * e;
  };
  auto bload = [&](int j, S &yj, S &qj, S &ln, S &xj) {
    const long k = p.base + j * st;
    yj = xout[k];
    qj = q[k];
    ln = j < n - 1 ? la[k + st] : S(0);
    xj = S(0);
    if constexpr (!FROM0) xj = xin[k];
  };
  int j = n - 1;
  for (; j - kUB + 1 >= 0; j -= kUB) {
    S yj[kUB], qj[kUB], ln[kUB], xj[kUB];
#pragma unroll
    for (int u = 0; u < kUB; ++u) bload(j - u, yj[u], qj[u], ln[u], xj[u]);
#pragma unroll
    for (int u = 0; u < kUB; ++u) back(j - u, yj[u], qj[u], ln[u], xj[u]);
  }
  for (; j >= 0; --j) {
    S yj, qj, ln, xj;
    bload(j, yj, qj, ln, xj);
    back(j, yj, qj, ln, xj);
  }
}

}  // namespace
