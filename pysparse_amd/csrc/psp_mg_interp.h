// psp_mg_interp.h -- operator-dependent interpolation of precon.multigrid: galerkin=True, interp='operator' (DESIGN.md
// section 9j is the normative text).  Part of psp_mg.hip's translation unit, included after psp_mg_line.h; it works on the
// stored levels (GLevel) and the level-operator policy (GOp) of psp_mg_galerkin.h.  What only this mode has: the weights
// of a level's prolongation derived from the level's own stencil (mg_weights_kernel), the Galerkin product with those
// weights (mg_galerkin_w_kernel), b_c = R (b - A x) and x += P e with them (mg_restrict_w_kernel, mg_prolong_w_kernel) and
// the dense product of the coarsest level as a launch of its own (mg_dense_kernel): such a handle has no tail launch.
//
// The weights of a level are 2^ND arrays over its fine points, slot-major in one allocation (slot s at W + s N).  Bit a of
// a slot number says which parent along axis a the weight belongs to: 0 the lower one -- coarse index i_a / 2 - 1 of an
// even fine index i_a, and the only parent (i_a - 1) / 2 of an odd one or i_a of an axis that is not coarsened --, 1 the
// upper one, coarse index i_a / 2 of an even fine index.  A slot whose parent does not exist holds 0.
//
// Every sum below has one fixed order, written where it is formed; no kernel uses atomics but the counter of fallback
// points, an integer whose value does not depend on the order of the additions.
namespace {

// the number (d0 + 1) + 3 (d1 + 1) + 9 (d2 + 1) of a member of {-1, 0, 1}^ND, and its components back
template <int ND>
constexpr int i_code(int d0, int d1, int d2) {
  return (d0 + 1) + (ND > 1 ? 3 * (d1 + 1) : 0) + (ND > 2 ? 9 * (d2 + 1) : 0);
}
template <int ND>
constexpr int i_comp(int code, int axis) {
  return axis == 0 ? code % 3 - 1 : axis == 1 ? (ND > 1 ? (code / 3) % 3 - 1 : 0) : (ND > 2 ? code / 9 - 1 : 0);
}

// One point of one round of a level's weights.  F = the axes on which the point lies between two coarse points (coarsened
// axis, even index), m = |F|; the launch of round `round` computes the points with m == round from the weights of the
// points with smaller m, which earlier launches wrote.
//   m = 0: 1 in slot 0.
//   m >= 1: the row S_p[d] (the diagonal; per stored offset the lower array at p and, for the upper coupling, the lower
//     array at the neighbour; absent entries 0) is collapsed onto the axes of F: T[delta] = sum of S_p[d] over the d with
//     d_a = delta_a on F, in ascending number of d (d0 fastest).  With T0 = T[0] finite and > 0, slot by slot,
//     w_p = 0 - sum over delta != 0 in ascending number, p + delta inside the grid, of (T[delta] / T0) * w_{p + delta}: the
//     quotient is rounded, then the product, then the sum.  Else the point takes the linear weights,
//     2^-m (sum over delta in {-1, 1}^F in ascending number, p + delta inside the grid, of w_{p + delta}), and is counted.
// The neighbour's slot: along an axis with delta_a != 0 the neighbour has an odd index and its only parent (slot bit 0) is
// p's lower parent for delta_a = -1 and p's upper one for delta_a = +1; along the other axes the neighbour has p's index
// and p's slot bit.
template <int ND, int NOFF>
__global__ __launch_bounds__(256) void mg_weights_kernel(GLevel S, long N, int round, double *W,
                                                         unsigned long long *__restrict__ fallbacks) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  constexpr int P3 = g_pow3(ND), NS = 1 << ND, C0 = i_code<ND>(0, 0, 0);
  const int n0 = S.a.n[0], n1 = S.a.n[1], n2 = S.a.n[2];
  int p0, p1, p2;
  mg_split<ND>(S.a, p, p0, p1, p2);
  const bool f0 = S.a.co[0] && !(p0 & 1), f1 = ND > 1 && S.a.co[1] && !(p1 & 1), f2 = ND > 2 && S.a.co[2] && !(p2 & 1);
  const int m = (int)f0 + (int)f1 + (int)f2;
  if (m != round) return;
  if (m == 0) {
    g_for<0, NS>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      W[(long)s * N + p] = s == 0 ? 1.0 : 0.0;
    });
    return;
  }
  // the row, every index a compile-time constant
  double v[P3];
  g_for<0, P3>([&](auto cc) { v[decltype(cc)::value] = 0.0; });
  v[C0] = S.diag[p];
  g_for<0, NOFF>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    constexpr int d0 = g_d(ND, NOFF, k, 0), d1 = g_d(ND, NOFF, k, 1), d2 = g_d(ND, NOFF, k, 2);
    const long o = d0 + (long)n0 * (d1 + (long)n1 * d2);
    if (g_in<d0>(p0, n0) && g_in<d1>(p1, n1) && g_in<d2>(p2, n2)) v[i_code<ND>(d0, d1, d2)] = S.lo[k][p];
    if (g_in<-d0>(p0, n0) && g_in<-d1>(p1, n1) && g_in<-d2>(p2, n2)) v[i_code<ND>(-d0, -d1, -d2)] = S.lo[k][p - o];
  });
  // the collapse
  double T[P3];
  g_for<0, P3>([&](auto tc) {
    constexpr int t = decltype(tc)::value;
    constexpr int t0 = i_comp<ND>(t, 0), t1 = i_comp<ND>(t, 1), t2 = i_comp<ND>(t, 2);
    double sum = 0.0;
    g_for<0, P3>([&](auto dc) {
      constexpr int d = decltype(dc)::value;
      constexpr int d0 = i_comp<ND>(d, 0), d1 = i_comp<ND>(d, 1), d2 = i_comp<ND>(d, 2);
      // per axis: on F the components agree, off F delta is 0
      constexpr bool can0 = d0 == t0 || t0 == 0, can1 = d1 == t1 || t1 == 0, can2 = d2 == t2 || t2 == 0;
      if constexpr (can0 && can1 && can2) {
        const bool ok0 = f0 ? d0 == t0 : t0 == 0, ok1 = f1 ? d1 == t1 : t1 == 0, ok2 = f2 ? d2 == t2 : t2 == 0;
        if (ok0 && ok1 && ok2) sum += v[d];
      }
    });
    T[t] = sum;
  });
  const double T0 = T[C0];
  const bool fine = T0 > 0.0 && T0 <= DBL_MAX;
  if (!fine) atomicAdd(fallbacks, 1ull);
  const double half_m = m == 1 ? 0.5 : m == 2 ? 0.25 : 0.125;
  g_for<0, NS>([&](auto sc) {
    constexpr int s = decltype(sc)::value;
    constexpr bool s0 = (s & 1) != 0, s1 = (s & 2) != 0, s2 = (s & 4) != 0;
    double acc = 0.0;
    // an upper parent exists only along the axes of F
    if ((!s0 || f0) && (!s1 || f1) && (!s2 || f2)) {
      g_for<0, P3>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        constexpr int t0 = i_comp<ND>(t, 0), t1 = i_comp<ND>(t, 1), t2 = i_comp<ND>(t, 2);
        // delta_a = -1 leads to the lower parent, +1 to the upper one
        constexpr bool fit = (t0 == 0 || (t0 > 0) == s0) && (t1 == 0 || (t1 > 0) == s1) && (t2 == 0 || (t2 > 0) == s2);
        if constexpr (t != C0 && fit) {
          const bool onF = (t0 == 0 || f0) && (t1 == 0 || f1) && (t2 == 0 || f2);
          // the linear weights come from the neighbours that differ along every axis of F
          const bool corner = (t0 != 0) == f0 && (t1 != 0) == f1 && (t2 != 0) == f2;
          if (onF && (fine || corner) && g_in<t0>(p0, n0) && g_in<t1>(p1, n1) && g_in<t2>(p2, n2)) {
            constexpr int sq = (t0 == 0 && s0 ? 1 : 0) | (t1 == 0 && s1 ? 2 : 0) | (t2 == 0 && s2 ? 4 : 0);
            const long q = p + t0 + (long)n0 * (t1 + (long)n1 * t2);
            const double wq = W[(long)sq * N + q];
            if (fine)
              acc += (T[t] / T0) * wq;
            else
              acc += wq;
          }
        }
      });
    }
    W[(long)s * N + p] = fine ? 0.0 - acc : half_m * acc;
  });
}

// One coarse point K of A_c = R A P with the weights W of the source level: the diagonal and the lower entries
// A_c[K, K + D], each the sum over the fine rows i with P[i, K] != 0 (ascending) and, within i, the fine columns j = i + f
// with A[i, j] stored and P[j, J] != 0 (ascending) of A[i, j] * ((P[i, K] * P[j, J]) * 2^-coarsened axes) -- the terms and
// the order of mg_galerkin_point, whose comment explains e, f, D, t and the compile-time pruning.  P[i, K] is the weight of
// i in the slot that names K: along a coarsened axis K is the upper parent of i = c - 1 (e = -1) and the lower or only one
// of i = c, c + 1; likewise J for j by t.  The running sum keeps its rounding errors (two-sum) and adds them at the end, as
// the chain of a box handle does and for its reason (section 9i); here it also keeps what the two products of a term lose,
// so that an entry is the exact sum of the exact products, rounded once: the weights of the next level are formed from
// these entries by a collapse that cancels, and amplify whatever error the entries carry (section 9j, "Conditioning").
template <int ND, int SNOFF>
__device__ __forceinline__ void mg_galerkin_w_point(const GLevel &S, const double *__restrict__ W, long N, long K,
                                                    double omega, const GOut &out, int *__restrict__ flag) {
  const int n0 = S.a.n[0], n1 = S.a.n[1], n2 = S.a.n[2];
  const int K0 = (int)(K % S.a.nc[0]), K1 = (int)((K / S.a.nc[0]) % S.a.nc[1]), K2 = (int)(K / S.a.nc[0] / S.a.nc[1]);
  const bool co0 = S.a.co[0], co1 = S.a.co[1], co2 = S.a.co[2];
  const int c0 = co0 ? 2 * K0 + 1 : K0, c1 = co1 ? 2 * K1 + 1 : K1, c2 = co2 ? 2 * K2 + 1 : K2;
  const long cl = c0 + (long)n0 * (c1 + (long)n1 * c2);
  const double rs = S.a.rs;
  constexpr int DN = g_full_noff(ND), P3 = g_pow3(ND);
  g_for<0, DN + 1>([&](auto dc) {
    constexpr int dk = decltype(dc)::value;  // 0: the diagonal; k + 1: the k-th lower offset
    constexpr int D0 = dk ? g_full_d(dk - 1, 0) : 0, D1 = dk ? g_full_d(dk - 1, 1) : 0, D2 = dk ? g_full_d(dk - 1, 2) : 0;
    double acc = 0.0, lost = 0.0;
    if (g_in<D0>(K0, S.a.nc[0]) && g_in<D1>(K1, S.a.nc[1]) && g_in<D2>(K2, S.a.nc[2])) {
      g_for<0, P3>([&](auto ec) {
        constexpr int ee = decltype(ec)::value;
        constexpr int e0 = ee % 3 - 1, e1 = ND > 1 ? (ee / 3) % 3 - 1 : 0, e2 = ND > 2 ? ee / 9 - 1 : 0;
        g_for<0, P3>([&](auto fc) {
          constexpr int ff = decltype(fc)::value;
          constexpr int f0 = ff % 3 - 1, f1 = ND > 1 ? (ff / 3) % 3 - 1 : 0, f2 = ND > 2 ? ff / 9 - 1 : 0;
          constexpr int t0 = e0 + f0 - 2 * D0, t1 = e1 + f1 - 2 * D1, t2 = e2 + f2 - 2 * D2;
          constexpr bool pc0 = t0 >= -1 && t0 <= 1, pc1 = t1 >= -1 && t1 <= 1, pc2 = t2 >= -1 && t2 <= 1;
          constexpr bool pn0 = e0 == 0 && f0 == D0, pn1 = e1 == 0 && f1 == D1, pn2 = e2 == 0 && f2 == D2;
          constexpr bool isdiag = f0 == 0 && f1 == 0 && f2 == 0;
          constexpr bool islower = f2 < 0 || (f2 == 0 && (f1 < 0 || (f1 == 0 && f0 < 0)));
          constexpr int slot = isdiag ? 0 : islower ? g_slot(ND, SNOFF, f0, f1, f2) : g_slot(ND, SNOFF, -f0, -f1, -f2);
          if constexpr ((pc0 || pn0) && (pc1 || pn1) && (pc2 || pn2) && slot >= 0) {
            const bool ok = (co0 ? pc0 : pn0) && (co1 ? pc1 : pn1) && (co2 ? pc2 : pn2);
            const int i0 = c0 + e0, i1 = c1 + e1, i2 = c2 + e2;
            if (ok && i0 < n0 && i1 < n1 && i2 < n2 && g_in<f0>(i0, n0) && g_in<f1>(i1, n1) && g_in<f2>(i2, n2)) {
              const int si = (co0 && e0 == -1 ? 1 : 0) | (co1 && e1 == -1 ? 2 : 0) | (co2 && e2 == -1 ? 4 : 0);
              const int sj = (co0 && t0 == -1 ? 1 : 0) | (co1 && t1 == -1 ? 2 : 0) | (co2 && t2 == -1 ? 4 : 0);
              const long il = cl + e0 + (long)n0 * (e1 + (long)n1 * e2);
              const long jl = il + f0 + (long)n0 * (f1 + (long)n1 * f2);
              double a;
              if constexpr (isdiag)
                a = S.diag[il];
              else if constexpr (islower)
                a = S.lo[slot][il];
              else
                a = S.lo[slot][jl];
              // the term and what its two products lose (fma gives the error of a product exactly; rs is a power of two)
              const double wi = W[(long)si * N + il], wj = W[(long)sj * N + jl];
              const double pw = wi * wj, epw = fma(wi, wj, -pw);
              const double w = pw * rs;
              const double t = a * w, et = fma(a, w, -t) + a * (epw * rs);
              const double sum = acc + t, bb = sum - acc;
              lost += ((acc - (sum - bb)) + (t - bb)) + et;
              acc = sum;
            }
          }
        });
      });
    }
    acc += lost;
    if constexpr (dk == 0) {
      out.diag[K] = acc;
      out.w[K] = omega / acc;
      if (!(acc > 0.0) || !(acc <= DBL_MAX)) *flag = 1;
    } else {
      out.lo[dk - 1][K] = acc;
    }
  });
}

template <int ND, int SNOFF>
__global__ __launch_bounds__(256) void mg_galerkin_w_kernel(GLevel S, const double *__restrict__ W, long N, long Nc,
                                                            double omega, GOut out, int *__restrict__ flag) {
  const long K = (long)blockIdx.x * 256 + threadIdx.x;
  if (K < Nc) mg_galerkin_w_point<ND, SNOFF>(S, W, N, K, omega, out, flag);
}

// b_c = R (b - A x) with R = P' / 2^coarsened axes: mg_restrict_kernel's tiles (the fine residuals of a tile of coarse
// points plus halo in LDS; they never reach memory), then per coarse point the gather over its <= 3^ND fine neighbours
// c + e, axis 2 outermost, each axis ascending: sum += W[slot of K at c + e] * r[c + e], and the sum times 2^-coarsened axes
// at the end.  A neighbour outside the grid is skipped.  Writes only b_c, which nothing of the launch reads.
template <class Op>
__global__ __launch_bounds__(kResThreads) void mg_restrict_w_kernel(typename Op::Level A, int t0, int t1, int t2, int g0n,
                                                                    int g1n, const double *__restrict__ W, long N,
                                                                    const double *__restrict__ x,
                                                                    const double *__restrict__ b,
                                                                    double *__restrict__ bc) {
  __shared__ double r[kResLds];
  const Op op(A);
  const MgLevelArg &L = op.geo();
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
    double v = 0;
    if (g0 < L.n[0] && g1 < L.n[1] && g2 < L.n[2]) {
      const long i = g0 + (long)L.n[0] * (g1 + (long)L.n[1] * g2);
      v = b[i] - op.ax(X, i, g0, g1, g2);
    }
    r[t] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= t0 * t1 * t2) return;
  const int j0 = t % t0, q = t / t0, j1 = q % t1, j2 = q / t1;
  if (J0 + j0 >= L.nc[0] || J1 + j1 >= L.nc[1] || J2 + j2 >= L.nc[2]) return;
  // local fine coordinates of the first neighbour along each axis and how many there are
  const int a0 = L.co[0] ? 2 * j0 : j0, m0 = L.co[0] ? 3 : 1;
  const int a1 = L.co[1] ? 2 * j1 : j1, m1 = L.co[1] ? 3 : 1;
  const int a2 = L.co[2] ? 2 * j2 : j2, m2 = L.co[2] ? 3 : 1;
  double sum = 0;
  for (int k2 = 0; k2 < m2; ++k2) {
    const int g2 = f2 + a2 + k2;
    if (g2 >= L.n[2]) continue;
    const int s2 = (L.co[2] && k2 == 0) ? 4 : 0;  // e = -1: the coarse point is the upper parent
    for (int k1 = 0; k1 < m1; ++k1) {
      const int g1 = f1 + a1 + k1;
      if (g1 >= L.n[1]) continue;
      const int s1 = (L.co[1] && k1 == 0) ? 2 : 0;
      for (int k0 = 0; k0 < m0; ++k0) {
        const int g0 = f0 + a0 + k0;
        if (g0 >= L.n[0]) continue;
        const int s0 = (L.co[0] && k0 == 0) ? 1 : 0;
        const long i = g0 + (long)L.n[0] * (g1 + (long)L.n[1] * g2);
        sum += W[(long)(s0 | s1 | s2) * N + i] * r[(a0 + k0) + F0 * ((a1 + k1) + F1 * (a2 + k2))];
      }
    }
  }
  bc[(J0 + j0) + (long)L.nc[0] * ((J1 + j1) + (long)L.nc[1] * (J2 + j2))] = sum * L.rs;
}

// the parents of a fine index along one axis: `lo` for slot bit 0, `hi` for slot bit 1 (-1: there is none)
struct IAxisSrc {
  int lo, hi;
};
__device__ __forceinline__ IAxisSrc i_axis_src(int co, int g, int nc) {
  IAxisSrc s;
  s.hi = -1;
  if (!co) {
    s.lo = g;
  } else if (g & 1) {
    s.lo = (g - 1) >> 1;
  } else {
    s.lo = (g >> 1) - 1;  // -1 at g = 0
    s.hi = (g >> 1) < nc ? (g >> 1) : -1;
  }
  return s;
}

// x += P e: per fine point the sum over its <= 2^ND parents in ascending slot number of W[slot] * e[parent], then
// x = x + sum.  Reads e, W and its own x, writes its own x.
__global__ __launch_bounds__(256) void mg_prolong_w_kernel(MgLevelArg L, long N, const double *__restrict__ W,
                                                           const double *__restrict__ e, double *__restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int i0, i1, i2;
  mg_split(L, i, i0, i1, i2);
  const IAxisSrc a0 = i_axis_src(L.co[0], i0, L.nc[0]), a1 = i_axis_src(L.co[1], i1, L.nc[1]),
                 a2 = i_axis_src(L.co[2], i2, L.nc[2]);
  double sum = 0;
  for (int b2 = 0; b2 < 2; ++b2) {
    const int j2 = b2 ? a2.hi : a2.lo;
    if (j2 < 0) continue;
    for (int b1 = 0; b1 < 2; ++b1) {
      const int j1 = b1 ? a1.hi : a1.lo;
      if (j1 < 0) continue;
      for (int b0 = 0; b0 < 2; ++b0) {
        const int j0 = b0 ? a0.hi : a0.lo;
        if (j0 < 0) continue;
        sum += W[(long)(b0 | 2 * b1 | 4 * b2) * N + i] * e[j0 + (long)L.nc[0] * (j1 + (long)L.nc[1] * j2)];
      }
    }
  }
  x[i] = x[i] + sum;
}

// the coarsest level: x = A^-1 b with the inverse formed at creation, row by row in ascending column order (the tail's
// dense product as a launch of its own); m <= 27
__global__ __launch_bounds__(64) void mg_dense_kernel(int m, const double *__restrict__ minv, const double *__restrict__ b,
                                                      double *__restrict__ x) {
  const int t = threadIdx.x;
  if (t >= m) return;
  double s = 0;
  for (int j = 0; j < m; ++j) s += minv[t * m + j] * b[j];
  x[t] = s;
}

}  // namespace
