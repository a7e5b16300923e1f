// psp_lobpcg.hip -- LOBPCG for the k smallest eigenpairs of A x = lambda M x (A symmetric, M symmetric positive definite or
// absent, K a symmetric positive definite preconditioner for A or absent) with every n-vector on the device (DESIGN.md 9f;
// no reference analogue: the reference's only eigensolver is jdsym).
//   * per iteration ONE block application of K (op_apply_block: the block V-cycle for a multigrid handle), ONE block
//     product with A and one with M -- where jdsym pays for the matrix and the preconditioner once per vector;
//   * the search space S = [X | P | W] and its images A S and M S are three column-major blocks of leading dimension
//     ld = n rounded up to even (so every column starts on 16 bytes); W sits behind P, so the Rayleigh-Ritz update
//     [X | P] <- S [C_x | C_p] is one in-place bv_rotate per block, with the same coefficients for the images;
//   * the dense n x m work is psp_bvec.hip: bv_gram (S' A S, S' M S, the projections of W), bv_resid (residuals, their
//     norms and the compaction of the active columns in one pass), bv_gemv (W -= X h), bv_rotate;
//   * the host keeps the projected problem only (m <= 3k <= 96): Cholesky of S' M S, reduction to standard form, the
//     cyclic-Jacobi routine of psp_jdsym.hip.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "psp_internal.h"

using namespace psp;

namespace {

constexpr int kLobMaxK = 32;
constexpr int kGenMax = 128;

struct PoolVecs {  // device vectors from the solvers' pool, given back on every way out
  std::vector<std::pair<double *, size_t>> held;
  ~PoolVecs() {
    for (auto &h : held) scratch_put(h.first, h.second);
  }
  int get(size_t count, double **out) {
    double *p = nullptr;
    PSP_TRY(scratch_get(count ? count : 1, &p));
    held.push_back({p, count ? count : 1});
    *out = p;
    return PSP_OK;
  }
};

bool is_multi(const psp_op *op) {
  if (!op) return false;
  if (op->kind == PSP_OP_CSR && op->csr && op->csr->multi) return true;
  if (op->kind == PSP_OP_JACOBI && op->jac && op->jac->multi) return true;
  return false;
}

// ---------------------------------------------------------------------- the projected problem (host, column-major)

// G = L L' in the lower triangle of the m x m matrix G (leading dimension m), in place.  A pivot that is not above
// m eps times its diagonal entry (or not finite) ends the factorisation: the index of that column, -1 when all passed.
int chol_lower(int m, double *G) {
  for (int j = 0; j < m; ++j) {
    const double g = G[(size_t)j * m + j];
    double d = g;
    for (int p = 0; p < j; ++p) d -= G[(size_t)p * m + j] * G[(size_t)p * m + j];
    if (!std::isfinite(d) || !(d > (double)m * DBL_EPSILON * std::fabs(g)) || !(g > 0.0)) return j;
    d = std::sqrt(d);
    G[(size_t)j * m + j] = d;
    for (int i = j + 1; i < m; ++i) {
      double s = G[(size_t)j * m + i];
      for (int p = 0; p < j; ++p) s -= G[(size_t)p * m + i] * G[(size_t)p * m + j];
      G[(size_t)j * m + i] = s / d;
    }
  }
  return -1;
}

// The generalised symmetric problem GA c = lambda GM c of order m: GA, GM (leading dimension ld) are symmetrised,
// GM = L L', L^-1 GA L^-T goes to the cyclic-Jacobi routine, C = L^-T V.  lambda ascending, C' GM C = I.
// false: GM is not (numerically) positive definite.
bool gen_ritz(int m, const double *GA, const double *GM, int ld, double *lambda, double *C, int ldc) {
  std::vector<double> L((size_t)m * m), B((size_t)m * m), V((size_t)m * m), s(m);
  for (int c = 0; c < m; ++c)
    for (int r = 0; r < m; ++r) {
      L[(size_t)c * m + r] = 0.5 * (GM[(size_t)c * ld + r] + GM[(size_t)r * ld + c]);
      B[(size_t)c * m + r] = 0.5 * (GA[(size_t)c * ld + r] + GA[(size_t)r * ld + c]);
    }
  if (chol_lower(m, L.data()) >= 0) return false;
  // B <- L^-1 B (every column), then B <- (L^-1 B')' = L^-1 GA L^-T
  for (int pass = 0; pass < 2; ++pass) {
    for (int c = 0; c < m; ++c) {
      double *b = &B[(size_t)c * m];
      for (int i = 0; i < m; ++i) {
        double sum = b[i];
        for (int p = 0; p < i; ++p) sum -= L[(size_t)p * m + i] * b[p];
        b[i] = sum / L[(size_t)i * m + i];
      }
    }
    for (int c = 0; c < m; ++c)
      for (int r = 0; r < c; ++r) std::swap(B[(size_t)c * m + r], B[(size_t)r * m + c]);
  }
  for (int c = 0; c < m; ++c)
    for (int r = 0; r < c; ++r) B[(size_t)c * m + r] = 0.5 * (B[(size_t)c * m + r] + B[(size_t)r * m + c]);  // upper triangle
  sym_jacobi_eig(m, B.data(), m, s.data(), V.data(), m);
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) {  // insertion sort, ties keep their order
    int pos = i;
    while (pos > 0 && s[order[pos - 1]] > s[i]) {
      order[pos] = order[pos - 1];
      --pos;
    }
    order[pos] = i;
  }
  for (int i = 0; i < m; ++i) {
    lambda[i] = s[order[i]];
    const double *v = &V[(size_t)order[i] * m];
    double *c = C + (size_t)i * ldc;
    for (int r = m - 1; r >= 0; --r) {  // L' c = v
      double sum = v[r];
      for (int p = r + 1; p < m; ++p) sum -= L[(size_t)r * m + p] * c[p];
      c[r] = sum / L[(size_t)r * m + r];
    }
  }
  return true;
}

// Cholesky-QR coefficients of a block with Gram matrix G (m x m, leading dimension m, symmetrised here): columns are
// taken in order, one whose pivot fails (dependent on the kept ones to m eps) is dropped.  T (m x m, column-major): column
// i holds the coefficients of the i-th kept, orthonormalised column (zero rows for dropped columns).  Returns the count.
int cholqr_factors(int m, const double *G, double *T) {
  std::vector<int> keep;
  std::vector<double> L((size_t)m * m, 0.0);  // row i of the kept set: L[i*m + p]
  for (int j = 0; j < m; ++j) {
    const double g = G[(size_t)j * m + j];
    if (!(g > 0.0) || !std::isfinite(g)) continue;
    const int nk = (int)keep.size();
    std::vector<double> l(nk + 1);
    double d = g;
    bool finite = true;
    for (int p = 0; p < nk; ++p) {
      double sum = 0.5 * (G[(size_t)keep[p] * m + j] + G[(size_t)j * m + keep[p]]);
      for (int q = 0; q < p; ++q) sum -= l[q] * L[(size_t)p * m + q];
      l[p] = sum / L[(size_t)p * m + p];
      d -= l[p] * l[p];
      finite = finite && std::isfinite(l[p]);
    }
    if (!finite || !(d > (double)m * 64.0 * DBL_EPSILON * g)) continue;
    l[nk] = std::sqrt(d);
    for (int p = 0; p <= nk; ++p) L[(size_t)nk * m + p] = l[p];
    keep.push_back(j);
  }
  const int nk = (int)keep.size();
  for (size_t i = 0; i < (size_t)m * m; ++i) T[i] = 0.0;
  // column i of L^-T is row i of L^-1: solve L' t = e_i
  for (int i = 0; i < nk; ++i) {
    std::vector<double> t(nk, 0.0);
    for (int r = i; r >= 0; --r) {
      double sum = r == i ? 1.0 : 0.0;
      for (int p = r + 1; p <= i; ++p) sum -= L[(size_t)p * m + r] * t[p];
      t[r] = sum / L[(size_t)r * m + r];
    }
    for (int r = 0; r <= i; ++r) T[(size_t)i * m + keep[r]] = t[r];
  }
  return nk;
}

// ---------------------------------------------------------------------- the solver

int fetch_now(const double *src_dev, size_t count, double *dst) {
  if (count == 0) return PSP_OK;
  PSP_HIP(hipMemcpyAsync(dst, src_dev, sizeof(double) * count, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

int upload_now(double *dst_dev, const double *src, size_t count) {
  if (count == 0) return PSP_OK;
  PSP_HIP(hipMemcpyAsync(dst_dev, src, sizeof(double) * count, hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

struct Lobpcg {
  const psp_op *A, *M, *K;
  long n, ld;
  int k;
  double *S = nullptr, *AS = nullptr, *MS = nullptr, *R = nullptr, *G = nullptr, *theta_dev = nullptr, *nrm_dev = nullptr;
  std::vector<double> hG, T;
  long products = 0, cycles = 0;

  double *col(double *block, int c) const { return block + (size_t)c * ld; }

  int apply(const psp_op *op, int cols, const double *X, double *Y) { return op_apply_block(op, cols, X, ld, Y, ld); }

  // one Cholesky-QR pass on `cols` columns at column c0 of S (M inner product): the columns that survive are compacted to
  // the front of the range.  MS's columns of the range are overwritten (M V) when M is given; *kept = the count.
  int cholqr(int c0, int cols, int *kept) {
    *kept = cols;
    if (cols <= 0) return PSP_OK;
    double *V = col(S, c0), *MV = col(MS, c0);
    if (M) PSP_TRY(apply(M, cols, V, MV));
    PSP_TRY(bv_gram(n, cols, V, ld, cols, MV, ld, G, cols));
    PSP_TRY(fetch_now(G, (size_t)cols * cols, hG.data()));
    const int nk = cholqr_factors(cols, hG.data(), T.data());
    if (nk > 0) PSP_TRY(bv_rotate(n, cols, V, ld, T.data(), cols, 0, nk, 0));
    *kept = nk;
    return PSP_OK;
  }

  // residuals of the k columns of X: R gets the columns with slot >= 0, res the norms
  int residuals(const double *theta, const int *slot, double *res) {
    PSP_TRY(upload_now(theta_dev, theta, (size_t)k));
    PSP_TRY(bv_resid(n, k, AS, ld, MS, ld, theta_dev, slot, R, ld, nrm_dev));
    PSP_TRY(fetch_now(nrm_dev, (size_t)k, res));
    for (int c = 0; c < k; ++c) res[c] = std::sqrt(res[c]);
    return PSP_OK;
  }
};

int lobpcg_run(const psp_op *A, const psp_op *M, const psp_op *K, int n_, int k, double tol, int itmax, const double *X0_host,
               int x0_cols, long ldx0, double *lambda_host, double *X_host, long ldx, double *res_host, int *kconv, int *it_out,
               int *restarts_out) {
  Lobpcg s;
  s.A = A, s.M = M, s.K = K, s.n = n_, s.ld = (long)n_ + (n_ & 1), s.k = k;
  const long n = s.n, ld = s.ld;
  const int mmax = 3 * k;
  PoolVecs mem;
  PSP_TRY(mem.get((size_t)mmax * ld, &s.S));
  PSP_TRY(mem.get((size_t)mmax * ld, &s.AS));
  if (M) PSP_TRY(mem.get((size_t)mmax * ld, &s.MS));
  else s.MS = s.S;
  PSP_TRY(mem.get((size_t)k * ld, &s.R));
  PSP_TRY(mem.get((size_t)2 * mmax * mmax, &s.G));
  PSP_TRY(mem.get((size_t)k + 16, &s.theta_dev));
  PSP_TRY(mem.get((size_t)k + 16, &s.nrm_dev));
  s.hG.assign((size_t)2 * mmax * mmax, 0.0);
  s.T.assign((size_t)mmax * mmax, 0.0);
  double *S = s.S, *AS = s.AS, *MS = s.MS, *R = s.R;
  std::vector<double> theta(k, 0.0), res(k, 0.0), lam(mmax), Cm((size_t)mmax * mmax), U((size_t)mmax * mmax), GA, GM;
  std::vector<int> slot(k), want(k);

  // ---- start: X0 as given, the other columns from the generator; M-orthonormal; Rayleigh-Ritz on X
  if (x0_cols > 0) {
    PSP_HIP(hipMemcpy2DAsync(S, sizeof(double) * ld, X0_host, sizeof(double) * ldx0, sizeof(double) * n, x0_cols,
                             hipMemcpyHostToDevice, stream()));
    PSP_HIP(hipStreamSynchronize(stream()));
  }
  for (int c = x0_cols; c < k; ++c) PSP_TRY(random_fill_dev(n, (unsigned long long)c * (unsigned long long)n, s.col(S, c)));
  for (int pass = 0; pass < 2; ++pass) {
    int kept = 0;
    PSP_TRY(s.cholqr(0, k, &kept));
    if (kept < k) return fail(PSP_EINVAL, "lobpcg: the start vectors are zero or depend on each other");
  }
  PSP_TRY(s.apply(A, k, S, AS));
  if (M) PSP_TRY(s.apply(M, k, S, MS));
  PSP_TRY(bv_gram(n, k, S, ld, k, AS, ld, s.G, k));
  PSP_TRY(bv_gram(n, k, S, ld, k, MS, ld, s.G + (size_t)k * k, k));
  PSP_TRY(fetch_now(s.G, (size_t)2 * k * k, s.hG.data()));
  if (!gen_ritz(k, s.hG.data(), s.hG.data() + (size_t)k * k, k, lam.data(), Cm.data(), k))
    return fail(PSP_ESINGULAR, "lobpcg: X' M X of the start block is not positive definite (is M?)");
  PSP_TRY(bv_rotate(n, k, S, ld, Cm.data(), k, 0, k, 0));
  PSP_TRY(bv_rotate_again(n, k, AS, ld, k, 0));
  if (M) PSP_TRY(bv_rotate_again(n, k, MS, ld, k, 0));
  for (int c = 0; c < k; ++c) theta[c] = lam[c];

  int np = 0, it = 0, restarts = 0;
  for (int c = 0; c < k; ++c) slot[c] = c;  // every column active
  for (;;) {
    // ---- 1. residuals; a column at or below tol is soft-locked: it stays in X and gets no W or P column
    PSP_TRY(s.residuals(theta.data(), slot.data(), res.data()));
    bool all = true;
    for (int c = 0; c < k; ++c) all = all && res[c] <= tol;
    if (all || it >= itmax) {
      // the way out: X M-orthonormal to rounding, A X and M X by explicit products, the test repeated on them
      int kept = 0;
      PSP_TRY(s.cholqr(0, k, &kept));
      if (kept < k) return fail(PSP_ESINGULAR, "lobpcg: the eigenvector block lost rank");
      PSP_TRY(s.apply(A, k, S, AS));
      if (M) PSP_TRY(s.apply(M, k, S, MS));
      for (int c = 0; c < k; ++c) slot[c] = -1;
      PSP_TRY(s.residuals(theta.data(), slot.data(), res.data()));
      all = true;
      for (int c = 0; c < k; ++c) all = all && res[c] <= tol;
      if (all || it >= itmax) break;
    }
    int na = 0;
    bool same = true;
    for (int c = 0; c < k; ++c) {
      want[c] = res[c] <= tol ? -1 : na++;
      same = same && want[c] == slot[c];
    }
    if (!same) {  // R holds another set of columns than the active ones: once more (the norms have the same bits)
      slot = want;
      PSP_TRY(s.residuals(theta.data(), slot.data(), res.data()));
    }
    std::vector<int> active;
    for (int c = 0; c < k; ++c)
      if (slot[c] >= 0) active.push_back(c);

    // ---- 2. W = K R, one block application
    const int w0 = k + np;
    double *W = s.col(S, w0);
    if (K) {
      PSP_TRY(s.apply(K, na, R, W));
      ++s.cycles;
    } else {
      PSP_HIP(hipMemcpyAsync(W, R, sizeof(double) * ((size_t)(na - 1) * ld + n), hipMemcpyDeviceToDevice, stream()));
    }
    // ---- 3. W M-orthogonal to X (twice), then M-orthonormal by Cholesky-QR (twice); dependent columns are dropped
    for (int pass = 0; pass < 2; ++pass) {
      PSP_TRY(bv_gram(n, k, MS, ld, na, W, ld, s.G, k));
      for (int c = 0; c < na; ++c) PSP_TRY(bv_gemv(n, k, S, ld, s.G + (size_t)c * k, -1.0, 1.0, s.col(W, c)));
    }
    for (int pass = 0; pass < 2 && na > 0; ++pass) PSP_TRY(s.cholqr(w0, na, &na));
    if (na == 0 && np == 0) break;  // nothing left to extend the space with: the block is as good as this method gets it
    // ---- 4. the images of W
    if (na > 0) {
      PSP_TRY(s.apply(A, na, W, s.col(AS, w0)));
      ++s.products;
      if (M) PSP_TRY(s.apply(M, na, W, s.col(MS, w0)));
    }
    // ---- 5. the projected pencil on S = [X | P | W]
    const int m = k + np + na;
    PSP_TRY(bv_gram(n, m, S, ld, m, AS, ld, s.G, m));
    PSP_TRY(bv_gram(n, m, S, ld, m, MS, ld, s.G + (size_t)m * m, m));
    PSP_TRY(fetch_now(s.G, (size_t)2 * m * m, s.hG.data()));
    const double *hGA = s.hG.data(), *hGM = s.hG.data() + (size_t)m * m;
    // ---- 6. Rayleigh-Ritz; when S' M S does not factor, again without P (a restart), at last on X alone
    std::vector<int> idx(m);
    for (int i = 0; i < m; ++i) idx[i] = i;
    bool solved = false;
    for (int attempt = 0; attempt < 3 && !solved; ++attempt) {
      if (attempt == 1) {
        if (np == 0) continue;
        ++restarts;
        idx.clear();
        for (int i = 0; i < k; ++i) idx.push_back(i);
        for (int i = w0; i < m; ++i) idx.push_back(i);
      } else if (attempt == 2) {
        idx.resize(k);
      }
      const int mm = (int)idx.size();
      GA.assign((size_t)mm * mm, 0.0);
      GM.assign((size_t)mm * mm, 0.0);
      for (int c = 0; c < mm; ++c)
        for (int r = 0; r < mm; ++r) {
          GA[(size_t)c * mm + r] = hGA[(size_t)idx[c] * m + idx[r]];
          GM[(size_t)c * mm + r] = hGM[(size_t)idx[c] * m + idx[r]];
        }
      std::vector<double> Cs((size_t)mm * mm);
      if (!gen_ritz(mm, GA.data(), GM.data(), mm, lam.data(), Cs.data(), mm)) continue;
      std::fill(Cm.begin(), Cm.end(), 0.0);
      for (int c = 0; c < k; ++c)
        for (int r = 0; r < mm; ++r) Cm[(size_t)c * m + idx[r]] = Cs[(size_t)c * mm + r];
      solved = true;
    }
    if (!solved) return fail(PSP_ESINGULAR, "lobpcg: X' M X is not positive definite in iteration %d", it + 1);
    // ---- 7. X <- S C_x; P <- the (P, W) part of the same combination for the active columns, M-normalised
    int npn = 0;
    for (int c = 0; c < k; ++c) memcpy(&U[(size_t)c * m], &Cm[(size_t)c * m], sizeof(double) * m);
    for (int a : active) {
      if (k + npn >= m) break;  // W lost columns: no more directions than the (P, W) part has
      double *u = &U[(size_t)(k + npn) * m];
      for (int r = 0; r < m; ++r) u[r] = r < k ? 0.0 : Cm[(size_t)a * m + r];
      double sq = 0.0;
      for (int c = k; c < m; ++c) {
        double t = 0.0;
        for (int r = k; r < m; ++r) t += 0.5 * (hGM[(size_t)c * m + r] + hGM[(size_t)r * m + c]) * u[r];
        sq += u[c] * t;
      }
      if (!(sq > 0.0) || !std::isfinite(sq)) continue;
      const double scale = 1.0 / std::sqrt(sq);
      if (!std::isfinite(scale)) continue;
      for (int r = k; r < m; ++r) u[r] *= scale;
      ++npn;
    }
    PSP_TRY(bv_rotate(n, m, S, ld, U.data(), m, 0, k + npn, 0));
    PSP_TRY(bv_rotate_again(n, m, AS, ld, k + npn, 0));
    if (M) PSP_TRY(bv_rotate_again(n, m, MS, ld, k + npn, 0));
    for (int c = 0; c < k; ++c) theta[c] = lam[c];
    np = npn;
    ++it;
  }

  int conv = 0;
  for (int c = 0; c < k; ++c) {
    lambda_host[c] = theta[c];
    res_host[c] = res[c];
    conv += res[c] <= tol ? 1 : 0;
  }
  *kconv = conv;
  *it_out = it;
  *restarts_out = restarts;
  PSP_HIP(hipMemcpy2DAsync(X_host, sizeof(double) * ldx, S, sizeof(double) * ld, sizeof(double) * n, k, hipMemcpyDeviceToHost,
                           stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  if (K && K->kind == PSP_OP_SSOR && K->ssor) PSP_TRY(ssor_error_check(K->ssor));
  return PSP_OK;
}

}  // namespace

extern "C" {

int psp_lobpcg(const psp_op_t *A, const psp_op_t *M, const psp_op_t *K, int n, int k, double tol, int itmax,
               const double *X0_host, int x0_cols, long ldx0, double *lambda_host, double *X_host, long ldx, double *res_host,
               int *kconv, int *it) {
  if (!A || !lambda_host || !X_host || !res_host || !kconv || !it) return fail(PSP_EINVAL, "psp_lobpcg: NULL argument");
  if (n <= 0) return fail(PSP_EINVAL, "lobpcg: n must be positive");
  if (k < 1 || k > kLobMaxK) return fail(PSP_EINVAL, "lobpcg: k = %d outside 1 .. %d", k, kLobMaxK);
  if ((long)3 * k > n) return fail(PSP_EINVAL, "lobpcg: 3 k = %d exceeds n = %d", 3 * k, n);
  if (!(0.0 < tol)) return fail(PSP_EINVAL, "lobpcg: tol must be positive");
  if (itmax < 0) return fail(PSP_EINVAL, "lobpcg: itmax must not be negative");
  if (x0_cols < 0 || x0_cols > k || (x0_cols > 0 && (!X0_host || ldx0 < n)))
    return fail(PSP_EINVAL, "lobpcg: X0 needs 0 .. k columns of leading dimension >= n");
  if (ldx < n) return fail(PSP_EINVAL, "lobpcg: ldx < n");
  if (A->n != n || (M && M->n != n) || (K && K->n != n)) return fail(PSP_EINVAL, "matrix, mass matrix or preconditioner shapes differ");
  if (is_multi(A) || is_multi(M) || is_multi(K)) return fail(PSP_EINVAL, "lobpcg does not run on a multi-device matrix");
  for (const psp_op *op : {A, M, K}) {
    const psp_csr *c = op_native_csr(op);
    if (c && c->nparts > 0) return fail(PSP_EINVAL, "lobpcg does not run on a matrix stored in parts");
  }
  if (cpu_mode())
    return fail(PSP_ENODEV, "psp_lobpcg: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  HandleLock lock;
  op_lock_add(lock, A);
  op_lock_add(lock, M);
  op_lock_add(lock, K);
  lock.lock();
  PSP_TRY(ensure_device());
  int restarts = 0;
  int rc = lobpcg_run(A, M, K, n, k, tol, itmax, X0_host, x0_cols, ldx0, lambda_host, X_host, ldx, res_host, kconv, it, &restarts);
  if (rc != PSP_OK) {
    (void)hipStreamSynchronize(stream());  // a failed call leaves nothing in flight behind it
    return rc;
  }
  note_solve("lobpcg", -1, -1, restarts);
  return rc;
}

int psp_debug_gen_ritz(int m, const double *GA_host, const double *GM_host, int ld, double *lambda_host, double *C_host) {
  if (m < 1 || m > kGenMax || !GA_host || !GM_host || !lambda_host || !C_host || ld < m)
    return fail(PSP_EINVAL, "psp_debug_gen_ritz: bad argument");
  if (!gen_ritz(m, GA_host, GM_host, ld, lambda_host, C_host, ld))
    return fail(PSP_ESINGULAR, "psp_debug_gen_ritz: GM is not positive definite");
  return PSP_OK;
}

}  // extern "C"
