// psp_recur.h -- the scalar recurrences of the Krylov solvers, one copy each.
//
// The few lines of IEEE-double arithmetic that turn reduced dot products into alpha, beta, the Givens rotation and
// the exit code, as the reference writes them (pcg.c, minres.c, cgs.c, bicgstab.c, qmrs.c of pysparse/itsolvers/src).
// Every loop of a solver -- host scalars, device-resident scalars, the batched columns, the single-kernel loops, the
// CPU mode -- calls these functions, so that all of them return the same info, iter, relres and iterates by
// construction: host and device are compiled with -ffp-contract=off, and sqrt, fabs and division are correctly
// rounded on both.  Plain structs and force-inlined host+device functions; no kernels, no launches.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#define PSP_RECUR __host__ __device__ __forceinline__

namespace psp {

// ====================================================================== PCG (pcg.c:91-166)

// One recurrence: a solve, or one column of a batched solve.  `it` is the iteration being worked on (1-based); info,
// iter and relres are written by the exit that ends the solve.
struct PcgCol {
  double rho, rho1, alpha, beta, normr, tolb, n2b, relres;
  int info, iter, stag, it, maxit;
};

// the state before the head of iteration 1 (pcg.c:70, :86-89): rho = 1 is what :99 saves as rho1
PSP_RECUR PcgCol pcg_begin(double n2b, double tolb, double normr0, int maxit) {
  PcgCol c = {};
  c.rho = 1.0;
  c.normr = normr0;
  c.tolb = tolb;
  c.n2b = n2b;
  c.info = -1;
  c.it = 1;
  c.maxit = maxit;
  return c;
}

// an exit (pcg.c:165-166); true for the callers' `if (...) break`
PSP_RECUR bool pcg_exit(PcgCol &c, int info, int iter) {
  c.info = info;
  c.iter = iter;
  c.relres = c.normr / c.n2b;
  return true;
}

// pcg.c:99-112: the head of iteration c.it once rho = r.z is known.  true: the solve has ended
PSP_RECUR bool pcg_head(PcgCol &c, double rho) {
  c.rho1 = c.rho;
  c.rho = rho;
  if (rho == 0.0) return pcg_exit(c, -2, c.it);  // pcg.c:101-104
  if (c.it > 1) {
    const double beta = rho / c.rho1;
    if (beta == 0.0) return pcg_exit(c, -6, c.it);  // pcg.c:109-112
    c.beta = beta;
  }
  return false;
}

// pcg.c:117-125 with pq = p.q.  true: the solve has ended
PSP_RECUR bool pcg_alpha(PcgCol &c, double pq) {
  if (pq == 0.0) return pcg_exit(c, -6, c.it);  // pcg.c:118-120
  c.alpha = c.rho / pq;
  if (c.alpha == 0.0) c.stag = 1;  // pcg.c:124-125
  return false;
}

// pcg.c:139, :146-166 with the norm of the updated residual (the loops on the GPU take the root of r.r, the CPU mode
// calls dnrm2) and what the stagnation scan of :127-138 found (looked at only while no stagnation is recorded).
// true: the solve has ended; false: c.it is the next iteration, whose head comes next
PSP_RECUR bool pcg_tail(PcgCol &c, double normr, bool scan_stagnated) {
  if (c.stag == 0) c.stag = scan_stagnated ? 1 : 0;
  c.normr = normr;
  if (normr <= c.tolb) return pcg_exit(c, 0, c.it);       // pcg.c:154-157
  if (c.stag == 1) return pcg_exit(c, -5, c.it);          // pcg.c:159-162
  if (c.it == c.maxit) return pcg_exit(c, -1, c.it + 1);  // pcg.c:165: the loop ran out
  c.it += 1;
  return false;
}

// ====================================================================== MINRES (minres.c:96-193)

// The Lanczos coefficients and the Givens rotation of the running iteration
struct MinresRot {
  double beta, beta_old, alpha, c, c_old, s, s_old, eta, norm_rmr;
  double c1, c2;             // Lanczos coefficients: alpha / beta, beta / beta_old
  double r1, r2, r3, c_eta;  // the w / x update (minres.c:172-180)
};

// minres.c:82-94 with beta = sqrt(v_hat . y)
PSP_RECUR MinresRot minres_begin(double beta0, double norm_r0) {
  MinresRot R = {};
  R.beta = beta0;
  R.beta_old = 1.0;
  R.c = 1.0;
  R.c_old = 1.0;
  R.eta = beta0;
  R.norm_rmr = norm_r0;
  return R;
}

// minres.c:114 (strict <) at the head of the iteration after `iter`.  1: it runs; 0 / -1: the loop is over, and that
// is the info of minres.c:196
PSP_RECUR int minres_loop_test(int iter, int it_max, double norm_rmr, double errtol, double norm_r0) {
  const bool conv = norm_rmr < errtol * norm_r0;
  return (iter >= it_max || conv) ? (conv ? 0 : -1) : 1;
}

// minres.c:129, :131 with alpha = v . Av
PSP_RECUR void minres_alpha(MinresRot &R, double alpha) {
  R.alpha = alpha;
  R.c1 = alpha / R.beta;
  R.c2 = R.beta / R.beta_old;
}

// minres.c:143-164, :180, :192 with vy = v_hat . y, then the loop test of :114 for the next iteration.
// 1: go on; -3 / -6: left before the w / x update of iteration `iter` (:144-146, :160-162); 0 / -1: the w / x update of
// iteration `iter` is the last thing to do
PSP_RECUR int minres_rotate(MinresRot &R, double vy, int iter, int it_max, double errtol, double norm_r0) {
  const double alpha = R.alpha;
  const double beta_old = R.beta;
  R.beta_old = beta_old;
  if (vy < 0.0) return -3;  // minres.c:143-146
  const double beta = sqrt(vy);
  R.beta = beta;
  // QR factorisation + Givens rotation (minres.c:151-164)
  const double c_oold = R.c_old, c_old = R.c, s_oold = R.s_old, s_old = R.s;
  R.c_old = c_old;
  R.s_old = s_old;
  const double r1_hat = c_old * alpha - c_oold * s_old * beta_old;
  const double r1 = sqrt(r1_hat * r1_hat + beta * beta);
  const double r2 = s_old * alpha + c_oold * c_old * beta_old;
  const double r3 = s_oold * beta_old;
  if (r1 == 0.0) return -6;  // minres.c:160-162
  const double c = r1_hat / r1;
  const double s = beta / r1;
  R.c = c;
  R.s = s;
  R.r1 = r1;
  R.r2 = r2;
  R.r3 = r3;
  R.c_eta = c * R.eta;  // minres.c:180
  R.eta = -s * R.eta;
  R.norm_rmr = R.norm_rmr * fabs(s);  // minres.c:192
  return minres_loop_test(iter, it_max, R.norm_rmr, errtol, norm_r0);
}

// ====================================================================== cgs / bicgstab / qmrs

// The scalars of a cgs / bicgstab / qmrs loop: registers r[], written by the reductions and by kry_step.  On the device
// the fused vector kernels read their coefficients from here (KryArg) and do nothing once status is set.
struct KryDev {
  double r[32];
  int status;  // 1: the loop is over -- every later kernel is a no-op
  int code;    // which way it ended (per solver)
  int iter, maxit;
};

enum KryOp {
  kCgsD, kCgsR,
  kBicgD1, kBicgTt, kBicgXr,
  kQmrsDelta0, kQmrsEps, kQmrsRho, kQmrsDelta,
};
// cgs registers
enum { CG_RHO = 0, CG_ALPHA, CG_BETA, CG_D, CG_RES, CG_RHONEW, CG_THR };
// bicgstab registers
enum { BI_RHO1 = 0, BI_RHO2, BI_ALPHA, BI_OMEGA, BI_BETA, BI_D1, BI_D2, BI_RR, BI_RHONEXT, BI_RES0, BI_TOL, BI_RES };
// qmrs registers
enum { QM_RHO0 = 0, QM_RHO1, QM_TAU, QM_C0, QM_C1, QM_EPS0, QM_XI1, QM_THETA0, QM_THETA, QM_ETA0, QM_DELTA, QM_CC, QM_BETA,
       QM_CC2, QM_RHO1INV, QM_ERR, QM_RESINIT, QM_TOL, QM_OUT };

PSP_RECUR void kry_end(KryDev *S, int code) {
  S->status = 1;
  S->code = code;
}

// bicgstab.c: head of an iteration (the do-loop's first statements), after the previous one decided to go on
PSP_RECUR void bicg_head(KryDev *S) {
  S->iter += 1;
  if (S->r[BI_RHO1] == 0.0) {
    kry_end(S, 3);  // "return" with info as initialised (-6)
    return;
  }
  S->r[BI_BETA] = (S->r[BI_RHO1] / S->r[BI_RHO2]) * (S->r[BI_ALPHA] / S->r[BI_OMEGA]);
}

// qmrs.c: head of an iteration, up to where delta = K v1 . v1 is needed (while test, ++iter, eps0 test) ...
PSP_RECUR void qmrs_head(KryDev *S) {
  if (!(S->r[QM_ERR] > S->r[QM_TOL] && S->iter < S->maxit)) {
    kry_end(S, 1);  // the loop test failed: normal end
    return;
  }
  S->iter += 1;
  if (S->r[QM_EPS0] == 0.0) kry_end(S, 6);
}
// ... and from there (delta test, cc).  The fused loops have delta from the previous pass and take both at once; the
// unfused loop applies K between the two
PSP_RECUR void qmrs_head_delta(KryDev *S) {
  if (S->status) return;
  if (S->r[QM_DELTA] == 0.0) {
    kry_end(S, 2);
    return;
  }
  S->r[QM_CC] = S->r[QM_XI1] * (S->r[QM_DELTA] / S->r[QM_EPS0]);
}
// qmrs.c: the tail of an iteration (the xi1 test, rho0, err, c0, theta0)
PSP_RECUR void qmrs_tail(KryDev *S) {
  double *r = S->r;
  if (r[QM_XI1] == 0.0) {
    kry_end(S, 6);
    return;
  }
  r[QM_RHO0] = r[QM_RHO1];
  r[QM_ERR] = r[QM_TAU] / r[QM_RESINIT];
  r[QM_C0] = r[QM_C1];
  r[QM_THETA0] = r[QM_THETA];
}

// cgs.c: the convergence test on r.r ...
PSP_RECUR bool cgs_converged(KryDev *S) {
  if (!(S->r[CG_RES] < S->r[CG_THR])) return false;
  kry_end(S, 1);
  return true;
}
// ... and, with r . r0 (the unfused loop forms it only now): beta, the for-loop's increment and test
PSP_RECUR void cgs_next(KryDev *S) {
  double *r = S->r;
  r[CG_BETA] = r[CG_RHONEW] / r[CG_RHO];
  r[CG_RHO] = r[CG_RHONEW];
  S->iter += 1;
  if (!(S->iter < S->maxit)) kry_end(S, 2);
}

// the recurrences that follow the reduction(s) of OP, on the registers the reduction wrote
template <int OP>
PSP_RECUR void kry_step(KryDev *S) {
  double *r = S->r;
  if constexpr (OP == kCgsD) {  // cgs.c: alpha = rho / (v . r0)
    r[CG_ALPHA] = r[CG_RHO] / r[CG_D];
  }
  if constexpr (OP == kCgsR) {
    if (!cgs_converged(S)) cgs_next(S);
  }
  if constexpr (OP == kBicgD1) r[BI_ALPHA] = r[BI_RHO1] / r[BI_D1];  // alpha = rho / (rhat . v)
  if constexpr (OP == kBicgTt) r[BI_OMEGA] = r[BI_D1] / r[BI_D2];    // omega = (t . s) / (t . t)
  if constexpr (OP == kBicgXr) {  // res, the omega == 0 return, the loop test, then the next iteration's head
    const double res = sqrt(r[BI_RR]);
    r[BI_RES] = res;
    if (r[BI_OMEGA] == 0.0) {
      kry_end(S, 4);
    } else {
      r[BI_RHO2] = r[BI_RHO1];
      r[BI_RHO1] = r[BI_RHONEXT];
      if (!((res / r[BI_RES0] > r[BI_TOL]) && (S->iter < S->maxit))) kry_end(S, 1);
      else bicg_head(S);
    }
  }
  if constexpr (OP == kQmrsDelta0) {  // first iteration: delta = K v1 . v1, then the head
    r[QM_DELTA] = r[QM_OUT];
    qmrs_head(S);
    qmrs_head_delta(S);
  }
  if constexpr (OP == kQmrsEps) {  // eps0 = g . t; beta = eps0 / delta
    r[QM_EPS0] = r[QM_OUT];
    r[QM_BETA] = r[QM_EPS0] / r[QM_DELTA];
  }
  if constexpr (OP == kQmrsRho) {  // qmrs.c: rho1 = ||v1||, theta, c1, eta0, tau, the coefficients of the d / x update
    const double rho1 = sqrt(r[QM_OUT]);
    const double beta = r[QM_BETA], c0 = r[QM_C0];
    r[QM_RHO1] = rho1;
    r[QM_XI1] = rho1;
    if (c0 * fabs(beta) == 0.0) {
      kry_end(S, 6);
      return;
    }
    const double theta = rho1 / (c0 * fabs(beta));
    const double c1 = 1.0 / sqrt(theta * theta + 1.0);
    r[QM_THETA] = theta;
    r[QM_C1] = c1;
    if (beta * (c0 * c0) == 0.0) {
      kry_end(S, 6);
      return;
    }
    r[QM_ETA0] = -r[QM_ETA0] * r[QM_RHO0] * (c1 * c1) / (beta * (c0 * c0));
    r[QM_TAU] = r[QM_TAU] * theta * c1;
    if (rho1 == 0.0) {
      kry_end(S, 6);
      return;
    }
    const double d1 = r[QM_THETA0] * c1;
    r[QM_CC2] = d1 * d1;
    r[QM_RHO1INV] = 1.0 / rho1;
  }
  if constexpr (OP == kQmrsDelta) {  // delta of the next iteration; the tail of this one; the next one's head
    r[QM_DELTA] = r[QM_OUT];
    qmrs_tail(S);
    if (S->status) return;
    qmrs_head(S);
    qmrs_head_delta(S);
  }
}

}  // namespace psp
