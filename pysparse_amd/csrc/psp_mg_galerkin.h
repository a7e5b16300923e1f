// psp_mg_galerkin.h -- the second mode of precon.multigrid: galerkin=True (DESIGN.md section 9d is the normative text).
// Part of psp_mg.hip's translation unit (included after the cycle kernels, which both modes share).  What only the
// stored mode has: the level's arrays (GLevel), the offset tables, (A_l x)[i] from the arrays (g_ax / g_ax_rt) with the
// level-operator policies GOp / GTailOp that hand them to the cycle kernels, the extraction and the Galerkin product.
//
// A is any symmetric 3- / 5- / 7-point operator on the grid (varying coefficients); the level operators are
// A_0 = A, A_{l+1} = R_l A_l P_l with section 9c's P and R, stored as symmetric stencils, offset-major: the diagonal
// array and one array per LOWER offset o (entry K holds A_l[K, K+o], 0 where that neighbour does not exist); the upper
// coupling of K is read as the lower one stored at K - o, so what the kernels apply is exactly symmetric.  Level 0
// carries the ND axis offsets, every other level the (3^ND - 1) / 2 lower members of {-1, 0, 1}^ND.  With stencil='box'
// (section 9i) A is any symmetric operator with that full pattern, 9 points in 2-D and 27 in 3-D, and level 0 is stored like
// the others.
//
// The lower offsets of the full pattern in their fixed order (ascending |o| = |d0 + n0 d1 + n0 n1 d2| on every grid with
// n0, n1 >= 3): d2 = 0, -1; within it d1 = +1, 0, -1; within it d0 = +1, 0, -1; the lexicographically negative ones.
namespace {

constexpr int kGMaxOff = 13;

// S: the scalar type of the stored arrays and of the cycle (float: section 9g, the arrays rounded once from the double ones)
template <class S>
struct GLevelT {
  MgLevelArgT<S> a;  // n, co, nc, rs as in the matrix-free mode (c, d, w are not used)
  int nd;            // axes of the level's index
  int noff;          // lower arrays: nd on level 0, (3^nd - 1) / 2 below
  const S *diag, *w;  // A_l[K, K] and omega / A_l[K, K]
  const S *lo[kGMaxOff];
  int od[kGMaxOff][3];  // the lower offsets' components, for the tail's run-time loop (g_ax_rt)
};
using GLevel = GLevelT<double>;

struct GOut {
  double *diag, *w, *lo[kGMaxOff];
};

template <class S>
__host__ __device__ inline const MgLevelArgT<S> &level_geo(const GLevelT<S> &G) {
  return G.a;
}

constexpr int g_full_noff(int nd) { return nd == 1 ? 1 : nd == 2 ? 4 : 13; }
constexpr int g_pow3(int nd) { return nd == 1 ? 3 : nd == 2 ? 9 : 27; }

// component `axis` of the k-th lower offset of the full pattern
constexpr int g_full_d(int k, int axis) {
  int idx = 0;
  for (int m2 = 0; m2 <= 1; ++m2)
    for (int d1 = 1; d1 >= -1; --d1)
      for (int d0 = 1; d0 >= -1; --d0) {
        const int d2 = -m2;
        const bool lower = d2 < 0 || (d2 == 0 && (d1 < 0 || (d1 == 0 && d0 < 0)));
        if (!lower) continue;
        if (idx == k) return axis == 0 ? d0 : axis == 1 ? d1 : d2;
        ++idx;
      }
  return 0;
}

// component `axis` of the k-th lower offset of a level of nd axes that stores noff arrays
constexpr int g_d(int nd, int noff, int k, int axis) {
  if (noff == nd && nd > 1) return axis == k ? -1 : 0;  // the axis offsets of level 0
  return g_full_d(k, axis);
}

// which array of such a level holds the lower offset (d0, d1, d2); -1: none (the coupling is structurally 0)
constexpr int g_slot(int nd, int noff, int d0, int d1, int d2) {
  for (int k = 0; k < noff; ++k)
    if (g_d(nd, noff, k, 0) == d0 && g_d(nd, noff, k, 1) == d1 && g_d(nd, noff, k, 2) == d2) return k;
  return -1;
}

// f(integral_constant<int, I>) for I = I0 .. N - 1, in this order, unrolled by the compiler's own instantiation: every
// offset below is a compile-time constant, no array of pointers or sums is ever indexed by a run-time value
template <int I, int N, class F>
__device__ __forceinline__ void g_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    g_for<I + 1, N>(f);
  }
}

template <int D>
__device__ __forceinline__ bool g_in(int v, int n) {
  if constexpr (D == 0)
    return true;
  else
    return (unsigned)(v + D) < (unsigned)n;
}

// (A_l x)[i]: the diagonal term, then per stored offset in its fixed order the lower and the upper neighbour
template <int ND, int NOFF, class S, class X>
__device__ __forceinline__ S g_ax(const GLevelT<S> &L, const X &x, long i, int i0, int i1, int i2) {
  S acc = L.diag[i] * x(i);
  const int n0 = L.a.n[0], n1 = L.a.n[1], n2 = L.a.n[2];
  g_for<0, NOFF>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    constexpr int d0 = g_d(ND, NOFF, k, 0), d1 = g_d(ND, NOFF, k, 1), d2 = g_d(ND, NOFF, k, 2);
    const long o = d0 + (long)n0 * (d1 + (long)n1 * d2);
    if (g_in<d0>(i0, n0) && g_in<d1>(i1, n1) && g_in<d2>(i2, n2)) acc += L.lo[k][i] * x(i + o);
    if (g_in<-d0>(i0, n0) && g_in<-d1>(i1, n1) && g_in<-d2>(i2, n2)) acc += L.lo[k][i - o] * x(i - o);
  });
  return acc;
}

// the same sum in the same order for a level whose shape is only known at run time (the tail, where L lives in global
// memory: the offsets and the array pointers are loads, nothing is indexed in registers)
template <class S, class X>
__device__ __forceinline__ S g_ax_rt(const GLevelT<S> &L, const X &x, int i, int i0, int i1, int i2) {
  S acc = L.diag[i] * x(i);
  const int n0 = L.a.n[0], n1 = L.a.n[1], n2 = L.a.n[2], noff = L.noff;
  for (int k = 0; k < noff; ++k) {
    const int d0 = L.od[k][0], d1 = L.od[k][1], d2 = L.od[k][2];
    const int o = d0 + n0 * (d1 + n1 * d2);
    const S *__restrict__ lo = L.lo[k];
    if ((unsigned)(i0 + d0) < (unsigned)n0 && (unsigned)(i1 + d1) < (unsigned)n1 && (unsigned)(i2 + d2) < (unsigned)n2)
      acc += lo[i] * x(i + o);
    if ((unsigned)(i0 - d0) < (unsigned)n0 && (unsigned)(i1 - d1) < (unsigned)n1 && (unsigned)(i2 - d2) < (unsigned)n2)
      acc += lo[i - o] * x(i - o);
  }
  return acc;
}

// One row of a stored level in registers, for the block kernels: the diagonal, omega / diagonal, and
// per stored offset the lower coupling (the array at i) and the upper one (the array at i - o), 0 where the neighbour
// does not exist (mlo / mup say which do).  WN: also omega / diagonal of every neighbour, which the fused first pass
// (xin = w .* b formed on the fly) multiplies the neighbours' b by.  Every index is a compile-time constant.
template <class S, int NOFF, bool WN>
struct GRow {
  S d, w;
  S lo[NOFF], up[NOFF];
  S wlo[WN ? NOFF : 1], wup[WN ? NOFF : 1];
  unsigned mlo, mup;
};

// The level-operator policies of the stored mode.  GOp: the launch-per-step kernels, the level's shape in the type (g_ax).
template <int ND, int NOFF, class S>
struct GOp {
  using Scalar = S;
  // level 0 stores the axis offsets only (in 1-D every level does); level 0 of a box handle (section 9i) is a full-pattern
  // level like the lower ones, and the launch layer picks its wide vectors by the level's number
  static constexpr bool kFinest = NOFF == ND;
  static constexpr int kNoff = NOFF;
  using Level = GLevelT<S>;
  const Level &G;
  __device__ __forceinline__ explicit GOp(const Level &g) : G(g) {}
  __device__ __forceinline__ const MgLevelArgT<S> &geo() const { return G.a; }
  template <class X>
  __device__ __forceinline__ S ax(const X &x, long i, int i0, int i1, int i2) const {
    return g_ax<ND, NOFF>(G, x, i, i0, i1, i2);
  }
  // "load the row, then apply it to a column": every load of a coefficient happens in load_row, ax_row reads only the
  // column (x(j, w_j) is the column's value at j; w_j = omega / diagonal at j, 0.0 unless the row was loaded with WN).
  // The terms and their order are g_ax's.
  template <bool WN>
  __device__ __forceinline__ GRow<S, NOFF, WN> load_row(long i, int i0, int i1, int i2) const {
    GRow<S, NOFF, WN> r;
    r.d = G.diag[i];
    r.w = G.w[i];
    r.mlo = r.mup = 0u;
    const int n0 = G.a.n[0], n1 = G.a.n[1], n2 = G.a.n[2];
    g_for<0, NOFF>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int d0 = g_d(ND, NOFF, k, 0), d1 = g_d(ND, NOFF, k, 1), d2 = g_d(ND, NOFF, k, 2);
      const long o = d0 + (long)n0 * (d1 + (long)n1 * d2);
      const bool inl = g_in<d0>(i0, n0) && g_in<d1>(i1, n1) && g_in<d2>(i2, n2);
      const bool inu = g_in<-d0>(i0, n0) && g_in<-d1>(i1, n1) && g_in<-d2>(i2, n2);
      r.lo[k] = inl ? G.lo[k][i] : S(0);
      r.up[k] = inu ? G.lo[k][i - o] : S(0);
      if (inl) r.mlo |= 1u << k;
      if (inu) r.mup |= 1u << k;
      if constexpr (WN) {
        r.wlo[k] = inl ? G.w[i + o] : S(0);
        r.wup[k] = inu ? G.w[i - o] : S(0);
      }
    });
    return r;
  }
  template <bool WN, class X>
  __device__ __forceinline__ S ax_row(const GRow<S, NOFF, WN> &r, const X &x, long i, int, int, int) const {
    S acc = r.d * x(i, r.w);
    const int n0 = G.a.n[0], n1 = G.a.n[1];
    g_for<0, NOFF>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      constexpr int d0 = g_d(ND, NOFF, k, 0), d1 = g_d(ND, NOFF, k, 1), d2 = g_d(ND, NOFF, k, 2);
      const long o = d0 + (long)n0 * (d1 + (long)n1 * d2);
      S wl = 0, wu = 0;
      if constexpr (WN) wl = r.wlo[k], wu = r.wup[k];
      if ((r.mlo >> k) & 1u) acc += r.lo[k] * x(i + o, wl);
      if ((r.mup >> k) & 1u) acc += r.up[k] * x(i - o, wu);
    });
    return acc;
  }
  __device__ __forceinline__ S w(long i) const { return G.w[i]; }
  __device__ __forceinline__ void split(long i, int &i0, int &i1, int &i2) const { mg_split<ND>(G.a, i, i0, i1, i2); }
};
// GTailOp: the tail, where the level stays in global memory (g_ax_rt) and only its geometry is copied into registers
template <class S>
struct GTailOp {
  using Scalar = S;
  using Level = GLevelT<S>;
  const Level &G;
  const MgLevelArgT<S> L;
  __device__ __forceinline__ explicit GTailOp(const Level &g) : G(g), L(g.a) {}
  __device__ __forceinline__ const MgLevelArgT<S> &geo() const { return L; }
  template <class X>
  __device__ __forceinline__ S ax(const X &x, long i, int i0, int i1, int i2) const {
    return g_ax_rt(G, x, (int)i, i0, i1, i2);
  }
  __device__ __forceinline__ S w(long i) const { return G.w[i]; }
  __device__ __forceinline__ void split(long i, int &i0, int &i1, int &i2) const { mg_split(L, i, i0, i1, i2); }
};
// omega / diagonal as mg_scale_kernel takes it
template <class S>
struct GW {
  using Scalar = S;
  const S *__restrict__ w;
  __device__ __forceinline__ S operator()(long i) const { return w[i]; }
};

// precision='single' (section 9g): the level's arrays -- the diagonal, omega / diagonal, then the lower arrays, `total`
// numbers of which the first `nchk` are the two that must be positive -- rounded once to float, round to nearest.  *flag
// is set when a diagonal or an omega / diagonal is not a normal positive float afterwards (it overflowed, or fell below
// FLT_MIN), or a coupling is not finite.
__global__ __launch_bounds__(256) void mg_round_kernel(long total, long nchk, const double *__restrict__ src,
                                                       float *__restrict__ dst, int *__restrict__ flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float v = (float)src[i];
  dst[i] = v;
  const bool ok = i < nchk ? (v >= FLT_MIN && v <= FLT_MAX) : (fabsf(v) <= FLT_MAX);
  if (!ok) *flag = 1;
}

// ------------------------------------------------------------------ creation: extraction and the Galerkin product

enum {
  kGBadOffset = 1,   // an entry at an offset that is no axis stride
  kGBadWrap = 2,     // an entry across a line end
  kGBadDup = 4,      // an entry stored twice
  kGBadDiag = 8,     // no diagonal, or one that is not finite and > 0
  kGBadSym = 16      // A[k, k+st] != A[k+st, k]
};

// one thread per row: checks every stored entry (section 9d, "accepted operators") and writes level 0's arrays; the
// lower arrays were zeroed before (a neighbour that is not stored counts as coupling 0)
__global__ __launch_bounds__(256) void mg_extract_csr_kernel(int n, int n0, int n1, int n2, double omega,
                                                             const int *__restrict__ ind, const int *__restrict__ col,
                                                             const double *__restrict__ val, GOut out,
                                                             int *__restrict__ bad) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int dim[3] = {n0, n1, n2};
  const long st[3] = {1, n0, (long)n0 * n1};
  const int g[3] = {r % n0, (r / n0) % n1, r / n0 / n1};
  unsigned seen = 0;
  int why = 0;
  double dg = 0.0;
  for (int k = ind[r]; k < ind[r + 1]; ++k) {
    const long off = (long)col[k] - r;
    const double v = val[k];
    if (off == 0) {
      if (seen & 1u) why |= kGBadDup;
      seen |= 1u;
      dg = v;
      continue;
    }
    int ax = -1, ga = 0, da = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (dim[a] > 1 && (off == st[a] || off == -st[a])) ax = a, ga = g[a], da = dim[a];
    if (ax < 0) {
      why |= kGBadOffset;
      continue;
    }
    const int up = off > 0;
    if (up ? ga >= da - 1 : ga <= 0) {
      why |= kGBadWrap;
      continue;
    }
    const unsigned bit = 1u << (1 + 2 * ax + up);
    if (seen & bit) why |= kGBadDup;
    seen |= bit;
    // the mirrored entry A[c, r], +0.0 where it is not stored, must have the same bits
    const int c = col[k];
    double m = 0.0;
    for (int q = ind[c]; q < ind[c + 1]; ++q)
      if (col[q] == r) m = val[q];
    if (__double_as_longlong(m) != __double_as_longlong(v)) why |= kGBadSym;
    if (!up) {
      if (ax == 0) out.lo[0][r] = v;
      if (ax == 1) out.lo[1][r] = v;
      if (ax == 2) out.lo[2][r] = v;
    }
  }
  if (!(seen & 1u) || !(dg > 0.0) || !(dg <= DBL_MAX)) why |= kGBadDiag;
  out.diag[r] = dg;
  out.w[r] = omega / dg;
  if (why) atomicOr(bad, why);
}

// stencil='box' (section 9i): the number (d0 + 1) + 3 (d1 + 1) + 9 (d2 + 1) of an offset in {-1, 0, 1}^3 -- 13 is the
// diagonal, the 13 numbers below it are the lower offsets (lexicographically negative, d2 first) -- and, four bits per
// number, the array of the full pattern that holds that lower offset (g_full_d's order)
constexpr int g_box_code(int d0, int d1, int d2) { return (d0 + 1) + 3 * (d1 + 1) + 9 * (d2 + 1); }
constexpr int kGBoxDiag = g_box_code(0, 0, 0);
constexpr unsigned long long g_box_slots() {
  unsigned long long t = 0;
  for (int k = 0; k < kGMaxOff; ++k)
    t |= (unsigned long long)k << (4 * g_box_code(g_full_d(k, 0), g_full_d(k, 1), g_full_d(k, 2)));
  return t;
}

// The checking and extraction pass of a box handle: one thread per row, which splits the row and every column into grid
// coordinates (no table of flat offsets: on a grid with n0 = 2 the flat offsets +1 and (-1, +1) coincide) and accepts an
// entry iff every per-axis difference lies in {-1, 0, 1} -- an entry that wraps across a line end has a difference beyond
// that, an axis of length 1 has difference 0.  Level 0 gets the full layout: all (3^ND - 1) / 2 lower arrays, zeroed
// before.  On a grid of fewer than 3 axes d2 (and d1) is 0 and only the first 4 (1) arrays, the ones the level has, are
// written.  The mirrored row is searched through at most 27 entries: a row with more stores an entry twice or outside the
// box and is refused on its own account.
__global__ __launch_bounds__(256) void mg_extract_box_kernel(int n, int n0, int n1, int n2, double omega,
                                                             const int *__restrict__ ind, const int *__restrict__ col,
                                                             const double *__restrict__ val, GOut out,
                                                             int *__restrict__ bad) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  constexpr unsigned long long slots = g_box_slots();
  const int r0 = r % n0, rq = r / n0, r1 = rq % n1, r2 = rq / n1;
  unsigned seen = 0;
  int why = 0;
  double dg = 0.0;
  for (int k = ind[r]; k < ind[r + 1]; ++k) {
    const int c = col[k];
    const double v = val[k];
    if ((unsigned)c >= (unsigned)n) {
      why |= kGBadOffset;
      continue;
    }
    const int cq = c / n0, d0 = c % n0 - r0, d1 = cq % n1 - r1, d2 = cq / n1 - r2;
    if (d0 < -1 || d0 > 1 || d1 < -1 || d1 > 1 || d2 < -1 || d2 > 1) {
      why |= kGBadOffset;
      continue;
    }
    const int code = g_box_code(d0, d1, d2);
    if ((seen >> code) & 1u) why |= kGBadDup;
    seen |= 1u << code;
    if (code == kGBoxDiag) {
      dg = v;
      continue;
    }
    // the mirrored entry A[c, r], +0.0 where it is not stored, must have the same bits
    double m = 0.0;
    const int qe = min(ind[c + 1], ind[c] + g_pow3(3));
    for (int q = ind[c]; q < qe; ++q)
      if (col[q] == r) m = val[q];
    if (__double_as_longlong(m) != __double_as_longlong(v)) why |= kGBadSym;
    if (code < kGBoxDiag) {
      const int slot = (int)((slots >> (4 * code)) & 15u);
      g_for<0, kGMaxOff>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        if (slot == s) out.lo[s][r] = v;
      });
    }
  }
  if (!((seen >> kGBoxDiag) & 1u) || !(dg > 0.0) || !(dg <= DBL_MAX)) why |= kGBadDiag;
  out.diag[r] = dg;
  out.w[r] = omega / dg;
  if (why) atomicOr(bad, why);
}

// One coarse point K of A_c = R A P: its diagonal and its lower entries A_c[K, K + D].  Each is the sum over the fine
// rows i with P[i, K] != 0 (ascending) and, within i, the fine columns j with A[i, j] stored and P[j, J] != 0 (ascending)
// of A[i, j] * (P[i, K] P[j, J] / 2^coarsened axes): the factor is an exact power of two.  Along a coarsened axis
// i = c + e with c = 2K + 1 the centre and e in {-1, 0, 1} (weight 1 at e = 0, else 1/2), j = i + f, and the centre of
// J = K + D lies at c + 2D: the weight of j is 1 where e + f = 2D, 1/2 where |e + f - 2D| = 1, else 0.  An axis that is
// not coarsened has P = I: e = 0 and f = D.  e, f and D are compile-time constants, so that the terms that cannot
// contribute are not compiled at all; SNOFF = the lower arrays of the source level (ND on level 0).
// COMP (the chain of a box handle, section 9i): the same terms in the same order, but the running sum keeps its rounding
// errors (Knuth's two-sum: s = acc + t exactly equals fl(s) + err) and adds them at the end, so that every entry is the
// exact sum rounded to within an ulp or two.  A constant-coefficient 27-point operator whose values are no binary fractions
// (the trilinear Laplacian: 8/3, -1/6, -1/12 and face couplings that cancel to 0) gets the same rounding error at every
// point of a level from the plain sum of up to 343 terms, a smooth perturbation that the cycle amplifies: measured 82 - 98
// eps max|z| in one application on (40, 36, 20) against 64 allowed, 1.5 - 1.9 with COMP (section 9i has the figures).
template <int ND, int SNOFF, bool COMP>
__device__ __forceinline__ void mg_galerkin_point(const GLevel &S, long K, double omega, const GOut &out,
                                                  int *__restrict__ flag) {
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
          // per axis: can the term contribute when the axis is coarsened (pc) / when it is not (pn)
          constexpr int t0 = e0 + f0 - 2 * D0, t1 = e1 + f1 - 2 * D1, t2 = e2 + f2 - 2 * D2;
          constexpr bool pc0 = t0 >= -1 && t0 <= 1, pc1 = t1 >= -1 && t1 <= 1, pc2 = t2 >= -1 && t2 <= 1;
          constexpr bool pn0 = e0 == 0 && f0 == D0, pn1 = e1 == 0 && f1 == D1, pn2 = e2 == 0 && f2 == D2;
          // where A[i, j] is stored: the diagonal, a lower array at i, or (an upper offset) the mirrored lower array at j
          constexpr bool isdiag = f0 == 0 && f1 == 0 && f2 == 0;
          constexpr bool islower = f2 < 0 || (f2 == 0 && (f1 < 0 || (f1 == 0 && f0 < 0)));
          constexpr int slot = isdiag ? 0 : islower ? g_slot(ND, SNOFF, f0, f1, f2) : g_slot(ND, SNOFF, -f0, -f1, -f2);
          if constexpr ((pc0 || pn0) && (pc1 || pn1) && (pc2 || pn2) && slot >= 0) {
            const bool ok = (co0 ? pc0 : pn0) && (co1 ? pc1 : pn1) && (co2 ? pc2 : pn2);
            const int i0 = c0 + e0, i1 = c1 + e1, i2 = c2 + e2;
            if (ok && i0 < n0 && i1 < n1 && i2 < n2 && g_in<f0>(i0, n0) && g_in<f1>(i1, n1) && g_in<f2>(i2, n2)) {
              const double w0 = co0 ? (e0 == 0 ? 1.0 : 0.5) * (t0 == 0 ? 1.0 : 0.5) : 1.0;
              const double w1 = co1 ? (e1 == 0 ? 1.0 : 0.5) * (t1 == 0 ? 1.0 : 0.5) : 1.0;
              const double w2 = co2 ? (e2 == 0 ? 1.0 : 0.5) * (t2 == 0 ? 1.0 : 0.5) : 1.0;
              const long il = cl + e0 + (long)n0 * (e1 + (long)n1 * e2);
              const long jl = il + f0 + (long)n0 * (f1 + (long)n1 * f2);
              double a;
              if constexpr (isdiag)
                a = S.diag[il];
              else if constexpr (islower)
                a = S.lo[slot][il];
              else
                a = S.lo[slot][jl];
              const double t = a * (w0 * w1 * w2 * rs);
              if constexpr (COMP) {
                const double sum = acc + t, bb = sum - acc;
                lost += (acc - (sum - bb)) + (t - bb);
                acc = sum;
              } else {
                acc += t;
              }
            }
          }
        });
      });
    }
    if constexpr (COMP) acc += lost;
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
__global__ __launch_bounds__(256) void mg_galerkin_kernel(GLevel S, long Nc, double omega, GOut out,
                                                          int *__restrict__ flag) {
  const long K = (long)blockIdx.x * 256 + threadIdx.x;
  if (K < Nc) mg_galerkin_point<ND, SNOFF, false>(S, K, omega, out, flag);
}

// the chain of a box handle of 2 or 3 axes, every source level of which has the full pattern
template <int ND>
__global__ __launch_bounds__(256) void mg_galerkin_box_kernel(GLevel S, long Nc, double omega, GOut out,
                                                              int *__restrict__ flag) {
  const long K = (long)blockIdx.x * 256 + threadIdx.x;
  if (K < Nc) mg_galerkin_point<ND, g_full_noff(ND), true>(S, K, omega, out, flag);
}

}  // namespace
