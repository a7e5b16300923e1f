// psp_jdsym.hip -- the Jacobi-Davidson eigensolver for A x = lambda M x (A, M symmetric; reference: pysparse/eigen/src/
// jdsym.c:207-621, correq.c, orthopack.c) with every n-vector on the device.
//   * the correction equation is a composite device operator (PSP_OP_CORREQ, correq_apply below: the eight cases of
//     correq.c:137-236); the six Krylov loops of psp_solvers.hip are written against op_apply on device vectors, so they
//     solve it unchanged (krylov_dev).  Its pcg / minres run the generic-operand loops; a fused inner loop is a follow-up.
//   * the dense n x m work (V' x, x -= V h, q = V u, V <- V U) goes through the block-vector kernels of psp_bvec.hip;
//     the coefficients of a projection stay on the device between the block dot product and the block update.
//   * H^-1 w of the preconditioned projections (k <= kmax unknowns) is a one-wave device kernel on the uploaded LU
//     factors: no host round trip inside an application of the operator.
//   * the j x j projected eigenproblem (j <= 128), its ordering and the LU of H are plain host C++ (no LAPACK here).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "psp_internal.h"

namespace psp {
int k_lin2(long n, double a, const double *x, double b, const double *y, double *z);
int k_scal(long n, double a, double *x);
}  // namespace psp

using namespace psp;

// ====================================================================== small dense host algebra

namespace {

constexpr int kRitzMax = 128;

// Eigenpairs of the symmetric j x j matrix whose upper triangle is in Mu (leading dimension ldm), by cyclic Jacobi
// rotations on a full copy; s ascending, U (ldu) the eigenvectors as columns.  An off-diagonal entry below
// eps ||M||_F / (100 j) is left alone: all of them together move an eigenvalue by less than 0.01 eps ||M||_F.
void jacobi_eig(int j, const double *Mu, int ldm, double *s, double *U, int ldu) {
  std::vector<double> a((size_t)j * j);
  double fro = 0.0;
  for (int c = 0; c < j; ++c)
    for (int r = 0; r <= c; ++r) {
      const double v = Mu[(size_t)c * ldm + r];
      a[(size_t)c * j + r] = v;
      a[(size_t)r * j + c] = v;
      fro += (r == c ? 1.0 : 2.0) * v * v;
    }
  fro = std::sqrt(fro);
  for (int c = 0; c < j; ++c)
    for (int r = 0; r < j; ++r) U[(size_t)c * ldu + r] = r == c ? 1.0 : 0.0;
  const double thr = DBL_EPSILON * fro / (100.0 * j);
  for (int sweep = 0; sweep < 100; ++sweep) {
    int rotations = 0;
    for (int p = 0; p < j - 1; ++p)
      for (int q = p + 1; q < j; ++q) {
        const double apq = a[(size_t)q * j + p];
        if (!(std::fabs(apq) > thr)) continue;
        ++rotations;
        const double app = a[(size_t)p * j + p], aqq = a[(size_t)q * j + q];
        const double zeta = (aqq - app) / (2.0 * apq);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), sn = t * c;
        for (int i = 0; i < j; ++i) {  // columns p, q of a
          const double aip = a[(size_t)p * j + i], aiq = a[(size_t)q * j + i];
          a[(size_t)p * j + i] = c * aip - sn * aiq;
          a[(size_t)q * j + i] = sn * aip + c * aiq;
        }
        for (int i = 0; i < j; ++i) {  // rows p, q
          const double api = a[(size_t)i * j + p], aqi = a[(size_t)i * j + q];
          a[(size_t)i * j + p] = c * api - sn * aqi;
          a[(size_t)i * j + q] = sn * api + c * aqi;
        }
        a[(size_t)q * j + p] = 0.0;
        a[(size_t)p * j + q] = 0.0;
        for (int i = 0; i < j; ++i) {
          const double uip = U[(size_t)p * ldu + i], uiq = U[(size_t)q * ldu + i];
          U[(size_t)p * ldu + i] = c * uip - sn * uiq;
          U[(size_t)q * ldu + i] = sn * uip + c * uiq;
        }
      }
    if (rotations == 0) break;
  }
  for (int i = 0; i < j; ++i) s[i] = a[(size_t)i * j + i];
}

// reorder the pairs by `order` (order[i] = which old pair comes i-th)
void permute_pairs(int j, const int *order, double *s, double *U, int ldu) {
  std::vector<double> s2(j), U2((size_t)j * j);
  for (int i = 0; i < j; ++i) {
    s2[i] = s[order[i]];
    memcpy(&U2[(size_t)i * j], U + (size_t)order[i] * ldu, sizeof(double) * j);
  }
  for (int i = 0; i < j; ++i) {
    s[i] = s2[i];
    memcpy(U + (size_t)i * ldu, &U2[(size_t)i * j], sizeof(double) * j);
  }
}

void stable_order(int j, const double *key, int *order) {  // insertion sort: j <= 128, ties keep their order
  for (int i = 0; i < j; ++i) {
    int pos = i;
    while (pos > 0 && key[order[pos - 1]] > key[i]) {
      order[pos] = order[pos - 1];
      --pos;
    }
    order[pos] = i;
  }
}

// the Ritz step (jdsym.c:293-302): eigenpairs of the upper triangle, in the order sorteig gives them (jdsym.c:769-815):
// ascending |s - tau|; strategy 1: every s < tau behind all others.  Ties keep ascending s.
void ritz(int j, const double *Mu, int ldm, double tau, int strategy, double *s, double *U, int ldu) {
  jacobi_eig(j, Mu, ldm, s, U, ldu);
  std::vector<int> order(j);
  std::vector<double> key(s, s + j);
  stable_order(j, key.data(), order.data());
  permute_pairs(j, order.data(), s, U, ldu);
  for (int i = 0; i < j; ++i) key[i] = (strategy == 1 && s[i] < tau) ? DBL_MAX : std::fabs(s[i] - tau);
  stable_order(j, key.data(), order.data());
  permute_pairs(j, order.data(), s, U, ldu);
}

// P H = L U in place, partial pivoting; piv[i]: the row exchanged with row i at step i (0-based)
int lu_factor(int k, double *H, int ldh, int *piv) {
  for (int c = 0; c < k; ++c) {
    int p = c;
    for (int r = c + 1; r < k; ++r)
      if (std::fabs(H[(size_t)c * ldh + r]) > std::fabs(H[(size_t)c * ldh + p])) p = r;
    piv[c] = p;
    if (H[(size_t)c * ldh + p] == 0.0) return PSP_ESINGULAR;
    if (p != c)
      for (int cc = 0; cc < k; ++cc) std::swap(H[(size_t)cc * ldh + c], H[(size_t)cc * ldh + p]);
    const double d = H[(size_t)c * ldh + c];
    for (int r = c + 1; r < k; ++r) H[(size_t)c * ldh + r] /= d;
    for (int cc = c + 1; cc < k; ++cc) {
      const double u = H[(size_t)cc * ldh + c];
      for (int r = c + 1; r < k; ++r) H[(size_t)cc * ldh + r] -= H[(size_t)c * ldh + r] * u;
    }
  }
  return PSP_OK;
}

// w := H^-1 w from the factors: the one sequence of operations of the host hook and the device kernel
__host__ __device__ inline void lu_solve_inplace(int k, const double *LU, int ldh, const int *piv, double *w) {
  for (int i = 0; i < k; ++i) {
    const int p = piv[i];
    if (p != i) {
      const double t = w[i];
      w[i] = w[p];
      w[p] = t;
    }
  }
  for (int i = 1; i < k; ++i) {
    double sum = w[i];
    for (int c = 0; c < i; ++c) sum -= LU[(size_t)c * ldh + i] * w[c];
    w[i] = sum;
  }
  for (int i = k - 1; i >= 0; --i) {
    double sum = w[i];
    for (int c = i + 1; c < k; ++c) sum -= LU[(size_t)c * ldh + i] * w[c];
    w[i] = sum / LU[(size_t)i * ldh + i];
  }
}

__global__ void lu_solve_kernel(int k, const double *__restrict__ LU, int ldh, const int *__restrict__ piv, double *w) {
  if (threadIdx.x == 0 && blockIdx.x == 0) lu_solve_inplace(k, LU, ldh, piv, w);
}

// uniform (0, 1) from splitmix64 of (seed, index)
__global__ void random_fill_kernel(long count, unsigned long long seed, unsigned long long first, double *out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long)gridDim.x * blockDim.x) {
    unsigned long long z = seed + (first + (unsigned long long)i) * 0xD6E8FEB86659FD93ull;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    out[i] = ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  }
}

int random_fill(long count, unsigned long long first, double *out) {
  if (count <= 0) return PSP_OK;
  long blocks = (count + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(random_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, stream(), count, 0x6A64'7379'6D21ull, first, out);
  PSP_LAUNCH_CHECK();
  return PSP_OK;
}

int copy_dev(long n, const double *src, double *dst) {
  if (src == dst) return PSP_OK;
  PSP_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream()));
  return PSP_OK;
}

// ---------------------------------------------------------------------- Gram-Schmidt on device blocks (orthopack.c)

// u -= Q_i (Qm_i' u) one column after the other (mgs / mgsm, orthopack.c:125-155); the coefficient never leaves the device
int mgs_dev(long n, int m, const double *Q, const double *Qm, double *u, double *h) {
  for (int i = 0; i < m; ++i) {
    PSP_TRY(bv_tdot(n, 1, Qm + (size_t)i * n, n, u, h));
    PSP_TRY(bv_gemv(n, 1, Q + (size_t)i * n, n, h, -1.0, 1.0, u));
  }
  return PSP_OK;
}

int dot_host(long n, const double *x, const double *y, double *h, double *out) {
  PSP_TRY(bv_tdot(n, 1, x, n, y, h));
  return fetch_scalars(h, 1, out);
}

int fetch_host(const double *src_dev, int count, double *dst) {
  if (count <= 0) return PSP_OK;
  if (count <= 16) return fetch_scalars(src_dev, count, dst);
  PSP_HIP(hipMemcpyAsync(dst, src_dev, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

// host values to the device, complete on return (the caller may change src at once)
int upload_now(double *dst_dev, const double *src, size_t count) {
  if (count == 0) return PSP_OK;
  PSP_HIP(hipMemcpyAsync(dst_dev, src, sizeof(double) * count, hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

// iterated classical Gram-Schmidt against the m columns of V (icgs, orthopack.c:39-68): again while the norm fell below
// half of what it was, at most five passes; *unrm = ||u|| afterwards
int icgs_dev(long n, int m, const double *V, double *u, double *h, double *unrm) {
  double sq;
  PSP_TRY(dot_host(n, u, u, h, &sq));
  *unrm = std::sqrt(sq);
  if (m == 0) return PSP_OK;
  bool isorth = false;
  for (int i = 0; !isorth && i < 5; ++i) {
    PSP_TRY(bv_tdot(n, m, V, n, u, h));
    PSP_TRY(bv_gemv(n, m, V, n, h, -1.0, 1.0, u));
    const double old = *unrm;
    PSP_TRY(dot_host(n, u, u, h, &sq));
    *unrm = std::sqrt(sq);
    isorth = *unrm > 0.5 * old;
  }
  return PSP_OK;
}

// the same in the M inner product (icgsm, orthopack.c:78-113); um = M u on return
int icgsm_dev(long n, int m, const double *V, const psp_op *M, double *u, double *um, double *h, double *unrm) {
  double sq;
  PSP_TRY(op_apply(M, u, um));
  PSP_TRY(dot_host(n, u, um, h, &sq));
  *unrm = std::sqrt(sq);
  if (m == 0) return PSP_OK;
  bool isorth = false;
  for (int i = 0; !isorth && i < 5; ++i) {
    PSP_TRY(bv_tdot(n, m, V, n, um, h));
    PSP_TRY(bv_gemv(n, m, V, n, h, -1.0, 1.0, u));
    PSP_TRY(op_apply(M, u, um));
    const double old = *unrm;
    PSP_TRY(dot_host(n, u, um, h, &sq));
    *unrm = std::sqrt(sq);
    isorth = *unrm > 0.5 * old;
  }
  return PSP_OK;
}

// ---------------------------------------------------------------------- the correction equation (correq.c)

// y = (A - theta M) x, w: work (correq.c:26-36);  y = (A - theta I) x (correq.c:38-45)
int a_theta(const psp_correq *ce, const double *x, double *y, double *w) {
  PSP_TRY(op_apply(ce->A, x, y));
  if (ce->M) {
    if (ce->theta != 0.0) {
      PSP_TRY(op_apply(ce->M, x, w));
      PSP_TRY(k_lin2(ce->n, 1.0, y, -ce->theta, w, y));
    }
    return PSP_OK;
  }
  return k_lin2(ce->n, 1.0, y, -ce->theta, x, y);
}

// y := (I - Amat Bmat') y (correq.c:55-64)
int project1(const psp_correq *ce, const double *Amat, const double *Bmat, double *y) {
  PSP_TRY(bv_tdot(ce->n, ce->k, Bmat, ce->n, y, ce->h));
  return bv_gemv(ce->n, ce->k, Amat, ce->n, ce->h, -1.0, 1.0, y);
}

// y := (I - Y H^-1 Qx') y (correq.c:72-91)
int project2(const psp_correq *ce, const double *Qx, double *y) {
  if (ce->k <= 0) return PSP_OK;
  PSP_TRY(bv_tdot(ce->n, ce->k, Qx, ce->n, y, ce->h));
  hipLaunchKernelGGL(lu_solve_kernel, dim3(1), dim3(64), 0, stream(), ce->k, ce->Hlu_dev, ce->kmax, ce->Hpiv_dev, ce->h);
  PSP_LAUNCH_CHECK();
  return bv_gemv(ce->n, ce->k, ce->Y, ce->n, ce->h, -1.0, 1.0, y);
}

// the right-hand side of the correction equation from the residual, in place (correq.c:99-135)
int correq_right(const psp_correq *ce, double *r) {
  const long n = ce->n;
  if (ce->optype == 2) {
    if (ce->M) return project1(ce, ce->Qm, ce->Q, r);
    return mgs_dev(n, ce->k, ce->Q, ce->Q, r, ce->h);
  }
  if (ce->K) {
    PSP_TRY(op_apply(ce->K, r, ce->w1));
    PSP_TRY(copy_dev(n, ce->w1, r));
    return project2(ce, ce->M ? ce->Qm : ce->Q, r);
  }
  if (ce->M) return project1(ce, ce->Q, ce->Qm, r);
  return mgs_dev(n, ce->k, ce->Q, ce->Q, r, ce->h);
}

}  // namespace

namespace psp {

// for psp_lobpcg.hip: the cyclic-Jacobi routine and the device generator of the start vectors, as jdsym uses them
void sym_jacobi_eig(int j, const double *Mu, int ldm, double *s, double *U, int ldu) { jacobi_eig(j, Mu, ldm, s, U, ldu); }
int random_fill_dev(long count, unsigned long long first, double *out) { return random_fill(count, first, out); }

int correq_apply(const psp_op *op, const double *x, double *y) {
  const psp_correq *ce = op->ce;
  if (!ce) return fail(PSP_EINVAL, "correction-equation operator without a system");
  const long n = ce->n;
  if (!op->ce_precon) {  // correq.c:137-191
    if (ce->optype == 2) {
      PSP_TRY(a_theta(ce, x, y, ce->w1));
      return ce->M ? project1(ce, ce->Qm, ce->Q, y) : project1(ce, ce->Q, ce->Q, y);
    }
    if (ce->K) {
      PSP_TRY(a_theta(ce, x, ce->w2, ce->w1));
      PSP_TRY(op_apply(ce->K, ce->w2, y));
      return project2(ce, ce->M ? ce->Qm : ce->Q, y);
    }
    PSP_TRY(a_theta(ce, x, y, ce->w1));
    return ce->M ? project1(ce, ce->Q, ce->Qm, y) : project1(ce, ce->Q, ce->Q, y);
  }
  // correq.c:193-236
  if (ce->optype == 2) {
    if (ce->K) {
      PSP_TRY(op_apply(ce->K, x, y));
      return project2(ce, ce->M ? ce->Qm : ce->Q, y);
    }
    if (ce->M) {
      PSP_TRY(copy_dev(n, x, y));
      return project1(ce, ce->Q, ce->Qm, y);
    }
  }
  return copy_dev(n, x, y);  // the preconditioner is inside the operator (or there is none)
}

}  // namespace psp

// ====================================================================== the driver

namespace {

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

struct DevInts {
  int *p = nullptr;
  ~DevInts() {
    if (p) (void)hipFree(p);
  }
};

bool is_multi(const psp_op *op) {
  if (!op) return false;
  if (op->kind == PSP_OP_CSR && op->csr && op->csr->multi) return true;
  if (op->kind == PSP_OP_JACOBI && op->jac && op->jac->multi) return true;
  return false;
}

int check_params(int n, const psp_jdsym_params_t *p, int *jmax_out, int *jmin_out) {
  if (n <= 0) return fail(PSP_EINVAL, "jdsym: n must be positive");
  if (!(0.0 < p->jdtol)) return fail(PSP_EINVAL, "jdsym: jdtol must be positive");
  if (!(0 < p->kmax && p->kmax <= n)) return fail(PSP_EINVAL, "jdsym: kmax = %d outside 1 .. n = %d", p->kmax, n);
  if (!(0 < p->jmax)) return fail(PSP_EINVAL, "jdsym: jmax must be positive");
  if (!(0 < p->jmin && p->jmin < p->jmax)) return fail(PSP_EINVAL, "jdsym: need 0 < jmin < jmax (jmin = %d, jmax = %d)", p->jmin, p->jmax);
  int jmax = p->jmax < n ? p->jmax : n;           // the reference's own unit test calls n = 3 with jmax = 25
  int jmin = p->jmin < jmax - 1 ? p->jmin : jmax - 1;
  if (jmax > kRitzMax) return fail(PSP_EINVAL, "jdsym: jmax = %d beyond %d", jmax, kRitzMax);
  if (p->itmax < 0) return fail(PSP_EINVAL, "jdsym: itmax must not be negative");
  if (!(0 < p->blksize && p->blksize <= p->kmax)) return fail(PSP_EINVAL, "jdsym: blksize = %d outside 1 .. kmax", p->blksize);
  if (p->blksize > jmin) return fail(PSP_EINVAL, "jdsym: blksize = %d > jmin = %d", p->blksize, jmin);
  if (p->blksize > jmax - jmin) return fail(PSP_EINVAL, "jdsym: blksize = %d > jmax - jmin = %d", p->blksize, jmax - jmin);
  if (p->blkwise != 0 && p->blkwise != 1) return fail(PSP_EINVAL, "jdsym: blkwise must be 0 or 1");
  if (p->optype != 1 && p->optype != 2) return fail(PSP_EINVAL, "jdsym: optype must be 1 (unsymmetric) or 2 (symmetric)");
  if (p->linitmax < 0) return fail(PSP_EINVAL, "jdsym: linitmax must not be negative");
  if (!(0.0 <= p->eps_tr)) return fail(PSP_EINVAL, "jdsym: eps_tr must not be negative");
  if (!(1.0 < p->toldecay)) return fail(PSP_EINVAL, "jdsym: toldecay must exceed 1");
  if (p->strategy != 0 && p->strategy != 1) return fail(PSP_EINVAL, "jdsym: strategy must be 0 or 1");
  if (p->linsolver < PSP_LIN_PCG || p->linsolver > PSP_LIN_CALLBACK) return fail(PSP_EINVAL, "jdsym: unknown linsolver %d", p->linsolver);
  if (p->linsolver == PSP_LIN_CALLBACK && !p->linsolve) return fail(PSP_EINVAL, "jdsym: PSP_LIN_CALLBACK without a callback");
  if (p->V0_host && p->v0_cols < 1) return fail(PSP_EINVAL, "jdsym: V0 without columns");
  *jmax_out = jmax;
  *jmin_out = jmin;
  return PSP_OK;
}

// x -> P x through the host (Jdsym_Proj): download, callback, upload
int project_host(const psp_jdsym_params_t *p, long n, double *v, std::vector<double> &hx, std::vector<double> &hy) {
  const size_t bytes = sizeof(double) * (size_t)n;
  PSP_HIP(hipMemcpyAsync(hx.data(), v, bytes, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  if (p->projector(p->projector_ctx, (int)n, hx.data(), hy.data()) != 0)
    return fail(PSP_ECALLBACK, "jdsym: the projector reported failure");
  PSP_HIP(hipMemcpyAsync(v, hy.data(), bytes, hipMemcpyHostToDevice, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  return PSP_OK;
}

int jdsym_run(const psp_op *A, const psp_op *M, const psp_op *K, int n_, const psp_jdsym_params_t *p, int jmax, int jmin,
              int *kconv, double *lambda, double *Q_host, int *it_outer, int *it_inner) {
  const long n = n_;
  const int kmax = p->kmax, blksize = p->blksize, blkwise = p->blkwise, itmax = p->itmax;
  double tau = p->tau;
  const double jdtol = p->jdtol;

  PoolVecs mem;
  double *V, *Q, *Qm = nullptr, *Y = nullptr, *Res, *temp1, *temp2, *hbuf, *cw1, *cw2, *ch, *Hlu_dev = nullptr;
  PSP_TRY(mem.get((size_t)n * jmax, &V));
  PSP_TRY(mem.get((size_t)n * kmax, &Q));
  PSP_TRY(mem.get((size_t)n * blksize, &Res));
  PSP_TRY(mem.get(n, &temp1));
  PSP_TRY(mem.get(n, &temp2));
  PSP_TRY(mem.get(n, &cw1));
  PSP_TRY(mem.get(n, &cw2));
  PSP_TRY(mem.get((size_t)jmax + kmax + 16, &hbuf));
  PSP_TRY(mem.get((size_t)kmax + 16, &ch));
  if (M) PSP_TRY(mem.get((size_t)n * kmax, &Qm));
  DevInts piv_dev;
  std::vector<double> H, Hlu;
  std::vector<int> Hpiv;
  if (K) {
    PSP_TRY(mem.get((size_t)n * kmax, &Y));
    PSP_TRY(mem.get((size_t)kmax * kmax, &Hlu_dev));
    PSP_HIP(hipMalloc((void **)&piv_dev.p, sizeof(int) * (size_t)kmax));
    H.assign((size_t)kmax * kmax, 0.0);
    Hlu.assign((size_t)kmax * kmax, 0.0);
    Hpiv.assign(kmax, 0);
  }
  std::vector<double> U((size_t)jmax * jmax, 0.0), Mh((size_t)jmax * jmax, 0.0), s(jmax, 0.0), resnrm(blksize, 0.0);
  std::vector<int> convind(blksize), keepind(blksize), solvestep(blksize, 1), actcorrits(blksize, 0);
  std::vector<double> hx, hy;
  if (p->projector || p->linsolver == PSP_LIN_CALLBACK) {
    hx.resize(n);
    hy.resize(n);
  }

  psp_correq ce;
  ce.n = n_;
  ce.kmax = kmax;
  ce.optype = p->optype;
  ce.A = A;
  ce.M = M;
  ce.K = K;
  ce.Q = Q;
  ce.Qm = Qm;
  ce.Y = Y;
  ce.Hlu_host = K ? Hlu.data() : nullptr;
  ce.Hpiv_host = K ? Hpiv.data() : nullptr;
  ce.Hlu_dev = Hlu_dev;
  ce.Hpiv_dev = piv_dev.p;
  ce.w1 = cw1;
  ce.w2 = cw2;
  ce.h = ch;
  psp_op ceA, ceK;
  ceA.kind = ceK.kind = PSP_OP_CORREQ;
  ceA.n = ceK.n = n_;
  ceA.ce = ceK.ce = &ce;
  ceK.ce_precon = 1;
  // the preconditioner half is the identity when optype is unsymmetric, or symmetric with neither K nor M (correq.c:224-231)
  const bool ceK_identity = p->optype != 2 || (!K && !M);

  // ---- initial search space (jdsym.c:214-257)
  int j = 0, k = 0;
  if (p->V0_host) {
    j = p->v0_cols < jmax ? p->v0_cols : jmax;
    std::vector<double> stage((size_t)n * j);
    for (int c = 0; c < j; ++c)
      for (long i = 0; i < n; ++i) stage[(size_t)c * n + i] = p->V0_host[i * p->v0_row_stride + c * p->v0_col_stride];
    PSP_TRY(upload_now(V, stage.data(), stage.size()));
  }
  if (j < blksize) {
    PSP_TRY(random_fill((long)(blksize - j) * n, 0, V + (size_t)j * n));
    j = blksize;
  }
  unsigned long long random_next = (unsigned long long)blksize * (unsigned long long)n;
  if (p->projector)
    for (int c = 0; c < j; ++c) PSP_TRY(project_host(p, n, V + (size_t)c * n, hx, hy));
  for (int c = 0; c < j; ++c) {
    double *v = V + (size_t)c * n, alpha;
    if (!M) {
      PSP_TRY(mgs_dev(n, c, V, V, v, hbuf));
      double sq;
      PSP_TRY(dot_host(n, v, v, hbuf, &sq));
      alpha = std::sqrt(sq);
    } else {
      PSP_TRY(icgsm_dev(n, c, V, M, v, temp1, hbuf, &alpha));
    }
    if (!(alpha > 0.0) || !std::isfinite(alpha))
      return fail(PSP_EINVAL, "jdsym: start vector %d is zero or depends on the ones before it", c);
    PSP_TRY(k_scal(n, 1.0 / alpha, v));
  }
  // interaction matrix M = V' A V, upper triangle (jdsym.c:261-267)
  for (int c = 0; c < j; ++c) {
    PSP_TRY(op_apply(A, V + (size_t)c * n, temp1));
    PSP_TRY(bv_tdot(n, c + 1, V, n, temp1, hbuf));
    PSP_TRY(fetch_host(hbuf, c + 1, &Mh[(size_t)c * jmax]));
  }

  int it = 0, nof_ce_its = 0;
  int actblksize = blksize;
  bool done = false;

  while (it < itmax && !done) {
    // ---- the projected eigenproblem (jdsym.c:293-302)
    ritz(j, Mh.data(), jmax, tau, p->strategy, s.data(), U.data(), jmax);

    // ---- convergence / restart (jdsym.c:317-521)
    bool found = true;
    while (found) {
      int conv = 0, keep = 0;
      for (int act = 0; act < actblksize; ++act) {
        double *q = Q + (size_t)(act + k) * n, *r = Res + (size_t)act * n;
        double *qm = Qm ? Qm + (size_t)(act + k) * n : nullptr, *y = Y ? Y + (size_t)(act + k) * n : nullptr;
        const double theta = s[act];
        PSP_TRY(upload_now(hbuf, &U[(size_t)act * jmax], j));
        PSP_TRY(bv_gemv(n, j, V, n, hbuf, 1.0, 0.0, q));  // the Ritz vector
        PSP_TRY(op_apply(A, q, r));
        if (!M) {
          PSP_TRY(k_lin2(n, 1.0, r, -theta, q, r));
        } else {
          PSP_TRY(op_apply(M, q, qm));
          PSP_TRY(k_lin2(n, 1.0, r, -theta, qm, r));
        }
        if (K) {  // y = K^-1 qm, then column and row k + act of H (jdsym.c:352-372)
          const double *mat = M ? Qm : Q, *vec = M ? qm : q;
          PSP_TRY(op_apply(K, vec, y));
          const int cnt = k + act + 1;
          std::vector<double> col(cnt), row(cnt);
          PSP_TRY(bv_tdot(n, cnt, mat, n, y, hbuf));
          PSP_TRY(fetch_host(hbuf, cnt, col.data()));
          PSP_TRY(bv_tdot(n, cnt, Y, n, vec, hbuf));
          PSP_TRY(fetch_host(hbuf, cnt, row.data()));
          for (int i = 0; i < cnt; ++i) H[(size_t)(k + act) * kmax + i] = col[i];
          for (int i = 0; i < cnt; ++i) H[(size_t)i * kmax + (k + act)] = row[i];
        }
        double sq;
        PSP_TRY(dot_host(n, r, r, hbuf, &sq));
        resnrm[act] = std::sqrt(sq);
        if (resnrm[act] < jdtol)
          convind[conv++] = act;
        else
          keepind[keep++] = act;
      }
      found = ((blkwise == 1 && conv == actblksize) || (blkwise == 0 && conv != 0)) &&
              (j > actblksize || k == kmax - actblksize);
      if (found) {
        for (int act = 0; act < conv; ++act) lambda[k + act] = s[convind[act]];
        {  // the Ritz values that stay: the kept ones of the block, then the rest
          std::vector<double> s2(s.begin(), s.begin() + j);
          for (int act = 0; act < keep; ++act) s[act] = s2[keepind[act]];
          for (int act = 0; act < j - actblksize; ++act) s[act + keep] = s2[act + actblksize];
        }
        // V <- [kept Ritz vectors | V U(:, actblksize .. j)]  (jdsym.c:415-426)
        PSP_TRY(bv_rotate(n, j, V, n, U.data(), jmax, actblksize, j - actblksize, keep));
        for (int act = 0; act < keep; ++act) PSP_TRY(copy_dev(n, Q + (size_t)(k + keepind[act]) * n, V + (size_t)act * n));
        for (int act = 0; act < conv; ++act) {
          const int from = k + convind[act], to = k + act;
          PSP_TRY(copy_dev(n, Q + (size_t)from * n, Q + (size_t)to * n));
          if (M) PSP_TRY(copy_dev(n, Qm + (size_t)from * n, Qm + (size_t)to * n));
          if (K) {
            PSP_TRY(copy_dev(n, Y + (size_t)from * n, Y + (size_t)to * n));
            for (int i = 0; i < to; ++i) H[(size_t)to * kmax + i] = H[(size_t)from * kmax + i];
            H[(size_t)to * (kmax + 1)] = H[(size_t)from * (kmax + 1)];
            for (int i = 0; i < to; ++i) H[(size_t)i * kmax + to] = H[(size_t)i * kmax + from];
          }
        }
        j -= conv;
        for (int c = 0; c < j; ++c)
          for (int r2 = 0; r2 < j; ++r2) {
            if (r2 <= c) Mh[(size_t)c * jmax + r2] = r2 == c ? s[c] : 0.0;
            U[(size_t)c * jmax + r2] = r2 == c ? 1.0 : 0.0;
          }
        if (p->strategy == 1)
          for (int act = 0; act < conv; ++act)
            if (lambda[k + act] > tau) tau = lambda[k + act];
        k += conv;
        actblksize = blksize < kmax - k ? blksize : kmax - k;
        if (k == kmax) {
          done = true;
          break;
        }
        {
          std::vector<int> st(solvestep);
          for (int act = 0; act < keep; ++act) solvestep[act] = st[keepind[act]];
          for (int act = keep; act < blksize; ++act) solvestep[act] = 1;
        }
      }
      // restart: keep the jmin best Ritz vectors (jdsym.c:504-519)
      if (j + actblksize > jmax) {
        const int jold = j;
        j = jmin;
        PSP_TRY(bv_rotate(n, jold, V, n, U.data(), jmax, 0, j, 0));
        for (int c = 0; c < j; ++c)
          for (int r2 = 0; r2 < j; ++r2) {
            if (r2 <= c) Mh[(size_t)c * jmax + r2] = r2 == c ? s[c] : 0.0;
            U[(size_t)c * jmax + r2] = r2 == c ? 1.0 : 0.0;
          }
      }
    }
    if (done) break;

    // ---- the correction equations (jdsym.c:534-612)
    if (K) {
      const int kk = k + actblksize;
      for (int c = 0; c < kk; ++c)
        for (int r2 = 0; r2 < kk; ++r2) Hlu[(size_t)c * kmax + r2] = H[(size_t)c * kmax + r2];
      if (lu_factor(kk, Hlu.data(), kmax, Hpiv.data()) != PSP_OK)
        return fail(PSP_ESINGULAR, "jdsym: H = Qm' K^-1 Qm (order %d) is singular", kk);
      PSP_TRY(upload_now(Hlu_dev, Hlu.data(), (size_t)kmax * kk));
      PSP_HIP(hipMemcpyAsync(piv_dev.p, Hpiv.data(), sizeof(int) * (size_t)kk, hipMemcpyHostToDevice, stream()));
      PSP_HIP(hipStreamSynchronize(stream()));
    }
    for (int act = 0; act < actblksize; ++act) {
      double *v = V + (size_t)j * n, *r = Res + (size_t)act * n;
      PSP_HIP(hipMemsetAsync(v, 0, sizeof(double) * (size_t)n, stream()));
      ce.k = k + actblksize;
      ce.theta = resnrm[act] < p->eps_tr ? s[act] : tau;  // the shift follows the Ritz value once it is trusted
      const double it_tol = std::pow(p->toldecay, (double)(-solvestep[act]));
      solvestep[act] += 1;
      PSP_TRY(correq_right(&ce, r));
      int info = 0, linit = 0;
      double linres = 0.0;
      if (p->linsolver == PSP_LIN_CALLBACK) {
        PSP_HIP(hipMemcpyAsync(hx.data(), r, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, stream()));
        PSP_HIP(hipStreamSynchronize(stream()));
        std::fill(hy.begin(), hy.end(), 0.0);
        if (p->linsolve(p->linsolve_ctx, &ceA, &ceK, n_, hx.data(), hy.data(), it_tol, p->linitmax, &info, &linit, &linres) != 0)
          return fail(PSP_ECALLBACK, "jdsym: the linear solver reported failure");
        PSP_TRY(upload_now(v, hy.data(), (size_t)n));
      } else {
        PSP_TRY(krylov_dev(p->linsolver, &ceA, ceK_identity ? nullptr : &ceK, n_, v, r, it_tol, p->linitmax, &info, &linit,
                           &linres));
      }
      nof_ce_its += linit;
      actcorrits[act] = linit;
      // (M-)orthogonalise against Q, project, (M-)orthonormalise against V (jdsym.c:588-602).  A correction that is
      // zero, not finite or inside span(V) (a solver that broke down) is replaced by a fresh pseudo-random direction --
      // the reference would divide by zero here.
      double alpha = 0.0;
      for (int attempt = 0; attempt < 3; ++attempt) {  // the solver's vector, then up to two replacements
        if (attempt > 0) {
          PSP_TRY(random_fill(n, random_next, v));
          random_next += (unsigned long long)n;
        }
        if (M) {
          PSP_TRY(mgs_dev(n, k + actblksize, Q, Qm, v, hbuf));
          if (p->projector) PSP_TRY(project_host(p, n, v, hx, hy));
          PSP_TRY(icgsm_dev(n, j, V, M, v, temp1, hbuf, &alpha));
        } else {
          PSP_TRY(mgs_dev(n, k + actblksize, Q, Q, v, hbuf));
          if (p->projector) PSP_TRY(project_host(p, n, v, hx, hy));
          PSP_TRY(icgs_dev(n, j, V, v, hbuf, &alpha));
        }
        if (alpha > 0.0 && std::isfinite(alpha)) break;
        alpha = 0.0;
      }
      if (!(alpha > 0.0)) return fail(PSP_EINVAL, "jdsym: no direction left to extend the search space with");
      PSP_TRY(k_scal(n, 1.0 / alpha, v));
      PSP_TRY(op_apply(A, v, temp1));
      PSP_TRY(bv_tdot(n, j + 1, V, n, temp1, hbuf));
      PSP_TRY(fetch_host(hbuf, j + 1, &Mh[(size_t)j * jmax]));
      ++j;
    }
    if (p->clvl >= 1) {
      printf("jdsym it %4d  k %3d  j %3d  res %9.2e  inner %4d  ritz", it + 1, k, j - blksize, resnrm[0], actcorrits[0]);
      for (int i = 0; i < (j - blksize < 5 ? j - blksize : 5); ++i) printf(" %9.2e", s[i]);
      printf("\n");
    }
    ++it;
  }

  *kconv = k;
  *it_outer = it;
  *it_inner = nof_ce_its;
  if (k > 0) PSP_HIP(hipMemcpyAsync(Q_host, Q, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost, stream()));
  PSP_HIP(hipStreamSynchronize(stream()));
  // an SSOR brick sweep that gave up reports through a sticky error word (psp_ssor.hip): one look covers every application
  if (K && K->kind == PSP_OP_SSOR && K->ssor) PSP_TRY(ssor_error_check(K->ssor));
  return PSP_OK;
}

}  // namespace

extern "C" {

int psp_jdsym(const psp_op_t *A, const psp_op_t *M, const psp_op_t *K, int n, const psp_jdsym_params_t *p, int *kconv,
              double *lambda_host, double *Q_host, int *it_outer, int *it_inner) {
  if (!A || !p || !kconv || !lambda_host || !Q_host || !it_outer || !it_inner) return fail(PSP_EINVAL, "psp_jdsym: NULL argument");
  if (A->n != n || (M && M->n != n) || (K && K->n != n))
    return fail(PSP_EINVAL, "matrix, preconditioner or projector shapes differ");
  int jmax = 0, jmin = 0;
  PSP_TRY(check_params(n, p, &jmax, &jmin));
  if (is_multi(A) || is_multi(M) || is_multi(K))
    return fail(PSP_EINVAL, "jdsym does not run on a multi-device matrix");
  if (cpu_mode())
    return fail(PSP_ENODEV, "psp_jdsym: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  HandleLock lock;
  op_lock_add(lock, A);
  op_lock_add(lock, M);
  op_lock_add(lock, K);
  lock.lock();
  PSP_TRY(ensure_device());
  int rc = jdsym_run(A, M, K, n, p, jmax, jmin, kconv, lambda_host, Q_host, it_outer, it_inner);
  // a failed call leaves nothing in flight behind it (its pool vectors are already back: their reuse on this thread is in
  // stream order either way)
  if (rc != PSP_OK) (void)hipStreamSynchronize(stream());
  return rc;
}

int psp_op_apply_host(const psp_op_t *op, const double *x_host, double *y_host) {
  if (!op || !x_host || !y_host) return fail(PSP_EINVAL, "psp_op_apply_host: NULL argument");
  if (cpu_mode())
    return fail(PSP_ENODEV, "psp_op_apply_host: not available with PSP_DEVICE=cpu (host mode covers csr / sss / jacobi / pcg / minres)");
  if (is_multi(op)) return fail(PSP_EINVAL, "psp_op_apply_host does not take a multi-device matrix");
  HandleLock lock;
  op_lock_add(lock, op);
  lock.lock();
  PSP_TRY(ensure_device());
  PoolVecs mem;
  double *x, *y;
  PSP_TRY(mem.get(op->n, &x));
  PSP_TRY(mem.get(op->n, &y));
  const size_t bytes = sizeof(double) * (size_t)op->n;
  PSP_HIP(hipMemcpyAsync(x, x_host, bytes, hipMemcpyHostToDevice, stream()));
  int rc = op_apply(op, x, y);
  if (rc == PSP_OK) {
    PSP_HIP(hipMemcpyAsync(y_host, y, bytes, hipMemcpyDeviceToHost, stream()));
  }
  PSP_HIP(hipStreamSynchronize(stream()));
  return rc;
}

int psp_debug_ritz(int j, const double *M_host, int ldm, double tau, int strategy, double *s_host, double *U_host, int ldu) {
  if (j < 1 || j > kRitzMax || !M_host || !s_host || !U_host || ldm < j || ldu < j || (strategy != 0 && strategy != 1))
    return fail(PSP_EINVAL, "psp_debug_ritz: bad argument");
  ritz(j, M_host, ldm, tau, strategy, s_host, U_host, ldu);
  return PSP_OK;
}

int psp_debug_lu_factor(int k, double *H_host, int ldh, int *piv) {
  if (k < 1 || !H_host || !piv || ldh < k) return fail(PSP_EINVAL, "psp_debug_lu_factor: bad argument");
  if (lu_factor(k, H_host, ldh, piv) != PSP_OK) return fail(PSP_ESINGULAR, "psp_debug_lu_factor: zero pivot");
  return PSP_OK;
}

int psp_debug_lu_solve(int k, const double *LU_host, int ldh, const int *piv, double *w_host) {
  if (k < 1 || !LU_host || !piv || !w_host || ldh < k) return fail(PSP_EINVAL, "psp_debug_lu_solve: bad argument");
  lu_solve_inplace(k, LU_host, ldh, piv, w_host);
  return PSP_OK;
}

}  // extern "C"
