// orbfe_lm_core.h -- what the four Levenberg-Marquardt solvers share (PoseOptimization, OptimizeSim3,
// LocalBundleAdjustment, OptimizeEssentialGraph): the lane count and the host group, the flag and stop
// codes, the record a host-driven backend reports through, g2o's OptimizationAlgorithmLevenberg::solve as
// a controller (LmCtl) with its host driver (lm_host_optimize), and Eigen's pivoted dense LDLT
// (lm_ldlt / lm_ldlt_solve) behind LinearSolverDense. Host/device inline functions, included by the four
// orbfe_*_core.h headers; tests/lm_ref.py is the same code in Python, line by line. Not part of the C ABI.
//
// Every operation is an IEEE double + - * / rounded separately (-ffp-contract=off), and the order of the
// operations below defines the solvers' bits. Deviations from g2o, deliberate:
//  - pow(2 rho - 1, 3) is x * x * x (no libm call);
//  - a trial whose chi2 is not finite is rejected as a failed solve is (tempChi = DBL_MAX);
//  - Eigen's pivot search is not followed over NaN: the callers fail the trial before the factorisation.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PO_HD __host__ __device__
#else
#define PO_HD
#endif
#include <stdint.h>

#include <cfloat>
#include <cmath>

#define PO_LANES 64
#define LM_FLAG_LARGE_STEP 1u /* == ORBFE_*_FLAG_LARGE_STEP: sin / cos of a rotation step above pi */
#define LM_FLAG_NONFINITE 2u  /* == ORBFE_*_FLAG_NONFINITE: a non-finite entry failed a trial */
#define LM_STOP_ALL 0         /* == ORBFE_*_STOP_*: every iteration ran */
#define LM_STOP_TERMINATE 1
#define LM_STOP_NBAD 2
#define LM_STOP_NO_EDGE 3
#define LM_STOP_FLAG 4 /* the stop flag read true at a poll (LocalBundleAdjustment only) */

// One round's trace of the two in-kernel solvers (orbfe_poseopt_round_t)
struct PoRound {
  int32_t n_active, iterations, trials, rejected_trials, stop, n_bad;
  double lambda, chi2;
};

// A group type G runs G::width of a problem's PO_LANES lanes at once and G::slots = PO_LANES / G::width
// of them one after the other: the host runs 1 and 64, the device (orbfe_lm_device.h) 64 and 1.
struct PoHostGroup {
  static constexpr int width = 1;
  static constexpr int slots = PO_LANES;
  PO_HD int lane() const { return 0; }
  PO_HD void sync() const {}
  // s: slots rows of N; the combined sums end in row 0
  template <int N>
  PO_HD void reduce(double (*s)[N]) const {
    for (int stride = PO_LANES / 2; stride >= 1; stride >>= 1)
      for (int l = 0; l < stride; l++)
        for (int k = 0; k < N; k++) s[l][k] = s[l][k] + s[l + stride][k];
  }
  // bit l of the result: bit c of lane l's word
  PO_HD uint64_t ballot(const uint64_t* bits, int c) const {
    uint64_t w = 0;
    for (int l = 0; l < PO_LANES; l++) w |= ((bits[l] >> c) & 1ull) << l;
    return w;
  }
};

PO_HD inline bool po_finite(double v) { return v - v == 0.0; }

// ---- the record of a host-driven backend --------------------------------------------------------------
// What the host reads per linearisation (chi, maxdiag where lambda starts from it) and per trial (chi,
// scale, fail, flags). The device writes it: the fields are naturally aligned.
struct LmRec {
  double chi, scale, maxdiag;
  int32_t fail;
  uint32_t flags;
};

PO_HD inline void lm_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (v) atomicOr(p, v);
#else
  *p |= v;
#endif
}

PO_HD inline void lm_fail(LmRec* rec, uint32_t flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(reinterpret_cast<uint32_t*>(&rec->fail), 1u);
  if (flag) atomicOr(&rec->flags, flag);
#else
  rec->fail = 1;
  rec->flags |= flag;
#endif
}

// ---- OptimizationAlgorithmLevenberg::solve ------------------------------------------------------------
// The caller keeps its loops (at most 10 trials per iteration) and calls these at the four points. In a
// kernel every lane holds the same LmCtl, so the control flow stays uniform.
struct LmCtl {
  double lambda, current, ini, ni, rho;
  int nbad, qmax;
};

// chi: the chi2 of the linearisation; lambda_init (computeLambdaInit) is read on the round's first only
PO_HD inline void lm_begin_iteration(LmCtl& c, double chi, bool first, double lambda_init) {
  c.ini = chi;
  c.current = chi;
  if (first) {
    c.lambda = lambda_init;
    c.ni = 2.0;
    c.nbad = 0;
  }
  c.rho = 0.0;
  c.qmax = 0;
}

// One trial at c.lambda: its chi2, whether the solve failed (ok2 == false) and computeScale's sum.
// -> accepted (discardTop: the trial becomes the estimate); otherwise pop, the estimate stands
PO_HD inline bool lm_trial(LmCtl& c, double chi_trial, bool failed, double scale) {
  const double temp = failed ? DBL_MAX : chi_trial;
  c.rho = c.current - temp;
  c.rho = c.rho / (scale + 1e-3);
  const bool accepted = c.rho > 0 && po_finite(temp);
  if (accepted) {
    const double y = 2 * c.rho - 1;
    double alpha = 1.0 - y * y * y;  // deviation: pow(2 * rho - 1, 3) as x * x * x
    alpha = 2.0 / 3.0 < alpha ? 2.0 / 3.0 : alpha;
    const double factor = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;
    c.lambda = c.lambda * factor;
    c.ni = 2.0;
    c.current = temp;
  } else {
    c.lambda = c.lambda * c.ni;
    c.ni = c.ni * 2;
  }
  c.qmax++;
  return accepted;
}

PO_HD inline bool lm_more_trials(const LmCtl& c) { return c.rho < 0 && c.qmax < 10; }

// -> LM_STOP_TERMINATE, LM_STOP_NBAD (three iterations in a row that gained less than ini / 1000), or
// LM_STOP_ALL to go on
PO_HD inline int lm_end_iteration(LmCtl& c) {
  if (c.qmax == 10 || c.rho == 0) return LM_STOP_TERMINATE;
  if ((c.ini - c.current) * 1e3 < c.ini) c.nbad++;
  else c.nbad = 0;
  return c.nbad >= 3 ? LM_STOP_NBAD : LM_STOP_ALL;
}

struct LmTrace {
  int32_t iterations, trials, rejected_trials, stop;
  double lambda, chi2;
  uint32_t flags;  // the trials' LmRec::flags, or-ed
};

struct LmNoPoll {
  bool operator()() const { return false; }
};

// SparseOptimizer::optimize(max_it) over a system that has an edge. A backend B supplies linearize, trial
// and accept; each returns 0 or an error status that ends the run. lambda starts at user_lambda where
// that is > 0 (setUserLambdaInit), else at 1e-5 * rec.maxdiag. poll() is optimize()'s terminate(): read
// before each iteration, and after a rejected trial only when another trial would follow.
template <class B, class Poll>
inline int lm_host_optimize(B& b, int max_it, double user_lambda, Poll& poll, LmTrace* tr) {
  LmTrace r = {0, 0, 0, LM_STOP_ALL, 0.0, 0.0, 0};
  LmCtl c = {0.0, 0.0, 0.0, 2.0, 0.0, 0, 0};
  int st = 0;
  for (int i = 0; i < max_it; i++) {
    if (poll()) {
      r.stop = LM_STOP_FLAG;
      break;
    }
    r.iterations++;
    LmRec rec;
    if ((st = b.linearize(&rec))) return st;
    lm_begin_iteration(c, rec.chi, i == 0, user_lambda > 0 ? user_lambda : 1e-5 * rec.maxdiag);
    bool more;
    do {
      if ((st = b.trial(c.lambda, &rec))) return st;
      r.flags |= rec.flags;
      r.trials++;
      if (lm_trial(c, rec.chi, rec.fail != 0, rec.scale)) {
        if ((st = b.accept())) return st;
      } else {
        r.rejected_trials++;
      }
      more = lm_more_trials(c);
      if (more && poll()) more = false;
    } while (more);
    r.stop = lm_end_iteration(c);
    if (r.stop != LM_STOP_ALL) break;
  }
  r.lambda = c.lambda, r.chi2 = c.current;
  *tr = r;
  return 0;
}

// ---- the dense N x N solve (one lane) -----------------------------------------------------------------
// EIGEN: LDLT<MatrixXd, Lower>::compute, unblocked and in place on the lower triangle of A (row r,
// column c at A[N r + c], only r >= c touched). Pivot: the largest |diagonal| of the trailing part, the
// first maximum wins; symmetric transpositions; the sign tracked for isPositive(). A, tr and temp are LDS
// on the device, so the pivot indices may address them.
template <int N>
PO_HD inline bool lm_ldlt(double* A, int* tr, double* temp) {
  const int n = N;
  int sign = 0;  // ZeroSign; 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
  for (int k = 0; k < n; k++) tr[k] = k;
  for (int k = 0; k < n; k++) {
    int big = k;
    double best = fabs(A[(N + 1) * k]);
    for (int j = k + 1; j < n; j++)
      if (fabs(A[(N + 1) * j]) > best) big = j, best = fabs(A[(N + 1) * j]);
    tr[k] = big;
    if (k != big) {
      const int p = big;  // k < p < N
      double tmp;
      for (int j = 0; j < k; j++) tmp = A[N * k + j], A[N * k + j] = A[N * p + j], A[N * p + j] = tmp;
      for (int i = p + 1; i < n; i++) tmp = A[N * i + k], A[N * i + k] = A[N * i + p], A[N * i + p] = tmp;
      tmp = A[(N + 1) * k], A[(N + 1) * k] = A[(N + 1) * p], A[(N + 1) * p] = tmp;
      for (int i = k + 1; i < p; i++) tmp = A[N * i + k], A[N * i + k] = A[N * p + i], A[N * p + i] = tmp;
    }
    if (k > 0) {
      for (int j = 0; j < k; j++) temp[j] = A[(N + 1) * j] * A[N * k + j];
      double s = A[N * k] * temp[0];
      for (int j = 1; j < k; j++) s = s + A[N * k + j] * temp[j];
      A[(N + 1) * k] = A[(N + 1) * k] - s;
      for (int i = k + 1; i < n; i++) {
        s = A[N * i] * temp[0];
        for (int j = 1; j < k; j++) s = s + A[N * i + j] * temp[j];
        A[N * i + k] = A[N * i + k] - s;
      }
    }
    const double akk = A[(N + 1) * k];
    const bool valid = fabs(akk) > 0.0;
    if (k == 0 && !valid) {  // the whole diagonal is zero: ZeroSign, isPositive()
      for (int j = 0; j < n; j++) tr[j] = j;
      return true;
    }
    if (valid)
      for (int i = k + 1; i < n; i++) A[N * i + k] = A[N * i + k] / akk;
    if (sign == 1) {
      if (akk < 0) sign = 2;
    } else if (sign == -1) {
      if (akk > 0) sign = 2;
    } else if (sign == 0) {
      if (akk > 0) sign = 1;
      else if (akk < 0) sign = -1;
    }
  }
  return sign == 1 || sign == 0;
}

// EIGEN: LDLT::solve on rhs (overwritten) into x: P b, the unit lower solve by columns, D^-1 (0 where
// |d| <= DBL_MIN), the transposed solve by dot products summed left to right, P^T. tr[k] is in k..N-1.
template <int N>
PO_HD inline void lm_ldlt_solve(const double* A, const int* tr, double* rhs, double* out) {
  const int n = N;
  double* x = rhs;
  double tmp;
  for (int k = 0; k < n; k++) tmp = x[k], x[k] = x[tr[k]], x[tr[k]] = tmp;
  for (int i = 0; i < n; i++)
    for (int r = i + 1; r < n; r++) x[r] = x[r] - x[i] * A[N * r + i];
  for (int i = 0; i < n; i++) x[i] = fabs(A[(N + 1) * i]) > DBL_MIN ? x[i] / A[(N + 1) * i] : 0.0;
  for (int i = n - 2; i >= 0; i--) {
    double s = A[N * (i + 1) + i] * x[i + 1];
    for (int j = i + 2; j < n; j++) s = s + A[N * j + i] * x[j];
    x[i] = x[i] - s;
  }
  for (int k = n - 1; k >= 0; k--) tmp = x[k], x[k] = x[tr[k]], x[tr[k]] = tmp;
  for (int i = 0; i < n; i++) out[i] = x[i];
}
