// orbfe_sim3.hip -- Sim3Solver on the GPU (include/orbfe_sim3.h): batched RANSAC over the
// correspondences of several loop-closure candidates.
//
//   k_sim3_hypotheses  one thread per (solver, hypothesis): swap-remove selection + ComputeSim3
//   k_sim3_inliers     one wavefront per hypothesis: CheckInliers over all correspondences
//   k_sim3_select      one thread per solver: find() replayed over the inlier counts
//
// One call stages every solver's inputs in one pinned buffer (one H2D copy), launches the three
// kernels on the handle's stream and takes every result down in one D2H copy. All offsets into the
// two buffers are formed on the host from counts it has checked against the handle's bounds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbfe_sim3.h"
#include "orbfe_device.h"
#include "orbfe_ktimer.h"
#include "orbfe_match_internal.h"
#include "orbfe_sim3_core.h"
#include "orbfe_stage.h"

#define SIM3_HYP_THREADS 64
#define SIM3_INL_THREADS 256
#define SIM3_INL_WAVES (SIM3_INL_THREADS / 64)

__global__ __launch_bounds__(SIM3_HYP_THREADS) void k_sim3_hypotheses(const uint8_t* __restrict__ in,
                                                                      uint8_t* __restrict__ res) {
  const Sim3Dev& P = reinterpret_cast<const Sim3Dev*>(in)[blockIdx.y];
  const int k = blockIdx.x * SIM3_HYP_THREADS + threadIdx.x;
  if (k >= P.n_eval) return;
  float T12[12], T21[12], R[9], t[3], s;
  if (P.has_hyp) {
    const float* h12 = reinterpret_cast<const float*>(in + P.in_t12) + 12 * (size_t)k;
    const float* h21 = reinterpret_cast<const float*>(in + P.in_t21) + 12 * (size_t)k;
    for (int i = 0; i < 12; i++) T12[i] = h12[i], T21[i] = h21[i];
    for (int i = 0; i < 9; i++) R[i] = 0.0f;
    for (int i = 0; i < 3; i++) t[i] = T12[4 * i + 3];
    s = 0.0f;
  } else {
    const int32_t* draw = reinterpret_cast<const int32_t*>(in + P.in_rand) + 3 * (size_t)k;
    const int d[3] = {draw[0], draw[1], draw[2]};  // checked by the host: 0 <= d[i] <= n-1-i
    int idx[3];
    sim3_select3(P.n, d, idx);
    const float* x1 = reinterpret_cast<const float*>(in + P.in_x1);
    const float* x2 = reinterpret_cast<const float*>(in + P.in_x2);
    float P1[3][3], P2[3][3];
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) {
        P1[r][c] = x1[3 * (size_t)idx[c] + r];
        P2[r][c] = x2[3 * (size_t)idx[c] + r];
      }
    sim3_compute(P1, P2, P.fix_scale, T12, T21, R, t, &s);
  }
  float* o12 = reinterpret_cast<float*>(res + P.o_t12) + 12 * (size_t)k;
  float* o21 = reinterpret_cast<float*>(res + P.o_t21) + 12 * (size_t)k;
  float* oR = reinterpret_cast<float*>(res + P.o_r) + 9 * (size_t)k;
  float* ot = reinterpret_cast<float*>(res + P.o_t) + 3 * (size_t)k;
  for (int i = 0; i < 12; i++) o12[i] = T12[i], o21[i] = T21[i];
  for (int i = 0; i < 9; i++) oR[i] = R[i];
  for (int i = 0; i < 3; i++) ot[i] = t[i];
  reinterpret_cast<float*>(res + P.o_s)[k] = s;
}

// Project (:379-400) of one point, then the squared distance to (u0, v0) in the order `sign`
// gives: err = (float)(d0*d0 + d1*d1) with the products and the sum in double.
__device__ __forceinline__ void sim3_project(const float* T, const float* K, float X, float Y, float Z, float& u,
                                             float& v) {
  const float px = gemv3_d(T, X, Y, Z, T[3]);
  const float py = gemv3_d(T + 4, X, Y, Z, T[7]);
  const float pz = gemv3_d(T + 8, X, Y, Z, T[11]);
  const float invz = 1 / pz;
  const float x = px * invz;
  const float y = py * invz;
  u = K[0] * x + K[2];
  v = K[1] * y + K[3];
}
__device__ __forceinline__ float sim3_sq_err(float d0, float d1) {
  return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

__global__ __launch_bounds__(SIM3_INL_THREADS) void k_sim3_inliers(const uint8_t* __restrict__ in,
                                                                   uint8_t* __restrict__ res) {
  const Sim3Dev& P = reinterpret_cast<const Sim3Dev*>(in)[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * SIM3_INL_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (k >= P.n_eval) return;
  float T12[12], T21[12], K1[4], K2[4];
  const float* g12 = reinterpret_cast<const float*>(res + P.o_t12) + 12 * (size_t)k;
  const float* g21 = reinterpret_cast<const float*>(res + P.o_t21) + 12 * (size_t)k;
  for (int i = 0; i < 12; i++) T12[i] = g12[i], T21[i] = g21[i];
  for (int i = 0; i < 4; i++) K1[i] = P.k1[i], K2[i] = P.k2[i];
  const float* x1 = reinterpret_cast<const float*>(in + P.in_x1);
  const float* x2 = reinterpret_cast<const float*>(in + P.in_x2);
  const float* max1 = reinterpret_cast<const float*>(in + P.in_max1);
  const float* max2 = reinterpret_cast<const float*>(in + P.in_max2);
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(res + P.o_mask) + (size_t)P.words * k;
  const int n = P.n;
  int count = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {  // c0 / 64 < words = ceil(n / 64)
    const int i = c0 + lane;
    bool inl = false;
    if (i < n) {
      const float X1 = x1[3 * (size_t)i], Y1 = x1[3 * (size_t)i + 1], Z1 = x1[3 * (size_t)i + 2];
      const float X2 = x2[3 * (size_t)i], Y2 = x2[3 * (size_t)i + 1], Z2 = x2[3 * (size_t)i + 2];
      // mvP1im1 / mvP2im2 (FromCameraToImage, :402-420)
      const float iz1 = 1 / Z1, iz2 = 1 / Z2;
      const float a1 = X1 * iz1, b1 = Y1 * iz1, a2 = X2 * iz2, b2 = Y2 * iz2;
      const float u11 = K1[0] * a1 + K1[2], v11 = K1[1] * b1 + K1[3];
      const float u22 = K2[0] * a2 + K2[2], v22 = K2[1] * b2 + K2[3];
      float u21, v21, u12, v12;
      sim3_project(T12, K1, X2, Y2, Z2, u21, v21);  // vP2im1
      sim3_project(T21, K2, X1, Y1, Z1, u12, v12);  // vP1im2
      const float err1 = sim3_sq_err(u11 - u21, v11 - v21);
      const float err2 = sim3_sq_err(u12 - u22, v12 - v22);
      inl = err1 < max1[i] && err2 < max2[i];
    }
    const unsigned long long word = __ballot(inl);
    count += __popcll(word);
    if (lane == 0) mask[c0 >> 6] = word;
  }
  if (lane == 0) reinterpret_cast<int32_t*>(res + P.o_cnt)[k] = count;
}

// find() (:208-212 over :139-206) per solver, in hypothesis order
__global__ __launch_bounds__(64) void k_sim3_select(const uint8_t* __restrict__ in, uint8_t* __restrict__ res,
                                                    int n_solvers) {
  const int sidx = threadIdx.x;
  if (sidx >= n_solvers) return;
  const Sim3Dev& P = reinterpret_cast<const Sim3Dev*>(in)[sidx];
  const int32_t* cnt = reinterpret_cast<const int32_t*>(res + P.o_cnt);
  int iterations = 0, best = -1, best_inliers = 0, accepted = -1, n_inliers = 0;
  while (iterations < P.max_its && iterations < P.n_eval) {
    const int k = iterations++;
    const int c = cnt[k];
    if (c >= best_inliers) {
      best_inliers = c;
      best = k;
      if (c > P.min_inliers) {
        accepted = k;
        n_inliers = c;
        break;
      }
    }
  }
  int32_t* o = reinterpret_cast<int32_t*>(res + P.o_sel);
  o[0] = accepted;
  o[1] = n_inliers;
  o[2] = best;
  o[3] = best_inliers;
  o[4] = (accepted < 0 && iterations >= P.max_its) ? 1 : 0;
  o[5] = iterations;
}

// ------------------------------------------------------------------------------------------
// host

struct Sim3Last {  // one solver of the last solve, for orbfe_sim3_iterate
  int n = 0, n_eval = 0, min_inliers = 0, max_its = 0, words = 0;
  bool launched = false;
  size_t o_mask = 0, o_t12 = 0, o_cnt = 0;
};

struct orbfe_sim3 : OrbfeDev {
  int S = 0, C = 0, H = 0;
  OrbfeStage in, res;  // inputs (one upload), results (one copy back); sized by sim3_plan_bounds
  std::vector<Sim3Last> last;
};

extern "C" int orbfe_sim3_create(int device, int max_solvers, int max_corr, int max_hyp, orbfe_sim3** out) {
  if (!out) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_create: bad argument");
  *out = nullptr;
  if (max_solvers < 1 || max_solvers > ORBFE_SIM3_MAX_SOLVERS || max_corr < 3 || max_corr > ORBFE_SIM3_MAX_CORR ||
      max_hyp < 1 || max_hyp > ORBFE_SIM3_MAX_HYP)
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_sim3_create: max_solvers in 1..64, max_corr in 3..4096, max_hyp in 1..1024");
  orbfe_sim3* h = new orbfe_sim3();
  h->S = max_solvers;
  h->C = max_corr;
  h->H = max_hyp;
  if (device < 0) {
    *out = h;
    return ORBFE_OK;
  }
  const int st = orbfe_dev_open(h, device, "orbfe_sim3_create");
  if (st != ORBFE_OK) {
    orbfe_sim3_destroy(h);
    return st;
  }
  size_t in_bytes, res_bytes;
  sim3_plan_bounds(h->S, h->C, h->H, &in_bytes, &res_bytes);
  ORBFE_CREATE_HIP(h, orbfe_sim3_destroy, orbfe_stage_alloc(&h->in, in_bytes, true));
  ORBFE_CREATE_HIP(h, orbfe_sim3_destroy, orbfe_stage_alloc(&h->res, res_bytes, true));
  *out = h;
  return ORBFE_OK;
}

extern "C" int orbfe_sim3_destroy(orbfe_sim3* h) {
  if (!h) return ORBFE_OK;
  if (orbfe_dev_close(h)) {
    orbfe_stage_free(&h->in);
    orbfe_stage_free(&h->res);
  }
  delete h;
  return ORBFE_OK;
}

// Argument checks of one solver; *n_eval = hypotheses to evaluate (0: n < min_inliers), *max_its
static int sim3_check_solver(const orbfe_sim3* h, const orbfe_sim3_solver_t* s, const orbfe_sim3_result_t* r,
                             int* n_eval, int* max_its) {
  if (s->n < 0 || s->n_hyp < 0 || s->min_inliers < 0 || s->max_iterations < 0 || !(s->probability >= 0.0) ||
      !(s->probability <= 1.0))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: bad solver parameter");
  if (s->n > h->C) return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_solve_batch: n above the handle's max_corr");
  if (r->hyp_capacity < 0 || r->mask_words < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: bad result capacity");
  *n_eval = 0;
  *max_its = std::max(1, s->max_iterations);
  if (s->n < s->min_inliers) return ORBFE_OK;  // bNoMore, nothing launched
  if (s->n < 3) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: a solver needs n >= 3");
  if (!s->x3dc1 || !s->x3dc2 || !s->sigma2_1 || !s->sigma2_2)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: null correspondence array");
  const bool has_hyp = s->hyp_t12 || s->hyp_t21;
  if (has_hyp && (!s->hyp_t12 || !s->hyp_t21))
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: hyp_t12 and hyp_t21 go together");
  if (!has_hyp && s->n_hyp > 0 && !s->rand_idx)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: null rand_idx");
  // mRansacMaxIts (:124-134): epsilon = (float)mRansacMinInliers / N
  *max_its = ransac_max_its(s->n, s->min_inliers, (float)s->min_inliers / s->n, s->probability, s->max_iterations);
  const int e = std::min(s->n_hyp, *max_its);
  if (e > h->H)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_solve_batch: more hypotheses than the handle's max_hyp");
  if (e > r->hyp_capacity || (e > 0 && r->inlier_mask && r->mask_words < (s->n + 63) / 64))
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_solve_batch: result capacity below the evaluated hypotheses");
  for (int i = 0; i < s->n; i++) {
    const float a = s->sigma2_1[i], b = s->sigma2_2[i];
    if (!(a >= 0.0f && a < 1e15f && b >= 0.0f && b < 1e15f))
      return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: sigma2 must be finite and >= 0");
  }
  if (!has_hyp && !ransac_check_draws(s->rand_idx, e, 3, s->n))
    return orbfe_set_error(ORBFE_ERR_ARG,
                           "orbfe_sim3_solve_batch: rand_idx outside 0 .. n-1-i for draw i of its iteration");
  *n_eval = e;
  return ORBFE_OK;
}

extern "C" int orbfe_sim3_solve_batch(orbfe_sim3* h, const orbfe_sim3_solver_t* solvers, int n_solvers,
                                      orbfe_sim3_result_t* results) {
  if (!h || !solvers || !results || n_solvers < 1)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_solve_batch: bad argument");
  if (n_solvers > h->S)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_solve_batch: more solvers than the handle's max_solvers");
  std::vector<int> n_eval(n_solvers), max_its(n_solvers);
  for (int i = 0; i < n_solvers; i++) {
    const int st = sim3_check_solver(h, &solvers[i], &results[i], &n_eval[i], &max_its[i]);
    if (st != ORBFE_OK) return st;
  }
  if (h->device < 0) return orbfe_set_error(ORBFE_ERR_STATE, "sim3 solver is host-only (device < 0)");
  h->last.assign(n_solvers, Sim3Last());
  // plan: the launched solvers' parameter records, then their inputs; results packed the same way
  std::vector<int> act;
  for (int i = 0; i < n_solvers; i++)
    if (n_eval[i] > 0) act.push_back(i);
  const int na = (int)act.size();
  OrbfeStage &in = h->in, &res = h->res;
  in.off = res.off = 0;
  Sim3Dev* dev;
  in.take<Sim3Dev>((size_t)std::max(na, 1), &dev);
  int max_e = 0;
  for (int a = 0; a < na; a++) {
    const orbfe_sim3_solver_t& s = solvers[act[a]];
    const size_t n = (size_t)s.n, e = (size_t)n_eval[act[a]];
    Sim3Dev d;
    memset(&d, 0, sizeof(d));
    d.n = s.n;
    d.n_eval = (int)e;
    d.fix_scale = s.fix_scale ? 1 : 0;
    d.min_inliers = s.min_inliers;
    d.max_its = max_its[act[a]];
    d.has_hyp = s.hyp_t12 ? 1 : 0;
    d.words = (s.n + 63) / 64;
    memcpy(d.k1, s.k1, sizeof(d.k1));
    memcpy(d.k2, s.k2, sizeof(d.k2));
    sim3_layout(in, res, n, e, d.has_hyp != 0, d);
    if (in.off > in.cap || res.off > res.cap)  // cannot happen within the handle's bounds
      return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_solve_batch: staging plan exceeds the handle's buffers");
    memcpy(in.h + d.in_x1, s.x3dc1, 12 * n);
    memcpy(in.h + d.in_x2, s.x3dc2, 12 * n);
    float* m1 = reinterpret_cast<float*>(in.h + d.in_max1);
    float* m2 = reinterpret_cast<float*>(in.h + d.in_max2);
    for (size_t i = 0; i < n; i++) {
      // mvnMaxError is std::vector<size_t>: truncated; the comparison converts it to float
      m1[i] = (float)(size_t)(9.210 * (double)s.sigma2_1[i]);
      m2[i] = (float)(size_t)(9.210 * (double)s.sigma2_2[i]);
    }
    if (d.has_hyp) {
      memcpy(in.h + d.in_t12, s.hyp_t12, 48 * e);
      memcpy(in.h + d.in_t21, s.hyp_t21, 48 * e);
    } else {
      memcpy(in.h + d.in_rand, s.rand_idx, 12 * e);
    }
    dev[a] = d;
    max_e = std::max(max_e, (int)e);
    Sim3Last& L = h->last[act[a]];
    L.launched = true;
    L.words = d.words;
    L.o_mask = d.o_mask;
    L.o_t12 = d.o_t12;
    L.o_cnt = d.o_cnt;
  }
  for (int i = 0; i < n_solvers; i++) {
    Sim3Last& L = h->last[i];
    L.n = solvers[i].n;
    L.n_eval = n_eval[i];
    L.min_inliers = solvers[i].min_inliers;
    L.max_its = max_its[i];
  }
  if (na > 0) {
    ORBFE_HIP_CHECK(hipSetDevice(h->device));
    int st;
    if ((st = orbfe_stage_upload(&in, h->stream)) != ORBFE_OK) return st;
    const uint8_t* din = in.d;
    uint8_t* dres = res.d;
    ORBFE_LAUNCH("k_sim3_hypotheses", k_sim3_hypotheses,
                 dim3((max_e + SIM3_HYP_THREADS - 1) / SIM3_HYP_THREADS, na), dim3(SIM3_HYP_THREADS), 0, h->stream, din,
                 dres);
    ORBFE_LAUNCH("k_sim3_inliers", k_sim3_inliers, dim3((max_e + SIM3_INL_WAVES - 1) / SIM3_INL_WAVES, na),
                 dim3(SIM3_INL_THREADS), 0, h->stream, din, dres);
    ORBFE_LAUNCH("k_sim3_select", k_sim3_select, dim3(1), dim3(64), 0, h->stream, din, dres, na);
    if ((st = orbfe_stage_download(&res, h->stream)) != ORBFE_OK) return st;
  }
  for (int i = 0; i < n_solvers; i++) {
    orbfe_sim3_result_t& r = results[i];
    r.n_evaluated = n_eval[i];
    r.ransac_max_its = max_its[i];
    r.accepted = -1;
    r.accepted_inliers = 0;
    r.best = -1;
    r.best_inliers = 0;
    r.no_more = solvers[i].n < solvers[i].min_inliers ? 1 : 0;
  }
  for (int a = 0; a < na; a++) {
    const Sim3Dev& d = dev[a];
    orbfe_sim3_result_t& r = results[act[a]];
    const size_t e = (size_t)d.n_eval;
    const uint8_t* base = res.h;
    if (r.n_inliers) memcpy(r.n_inliers, base + d.o_cnt, 4 * e);
    if (r.t12) memcpy(r.t12, base + d.o_t12, 48 * e);
    if (r.t21) memcpy(r.t21, base + d.o_t21, 48 * e);
    if (r.r12) memcpy(r.r12, base + d.o_r, 36 * e);
    if (r.tr12) memcpy(r.tr12, base + d.o_t, 12 * e);
    if (r.s12) memcpy(r.s12, base + d.o_s, 4 * e);
    if (r.inlier_mask) orbfe_unpack_masks(r.inlier_mask, r.mask_words, base + d.o_mask, d.words, e);
    const int32_t* sel = reinterpret_cast<const int32_t*>(base + d.o_sel);
    r.accepted = sel[0];
    r.accepted_inliers = sel[1];
    r.best = sel[2];
    r.best_inliers = sel[3];
    r.no_more = sel[4];
  }
  return ORBFE_OK;
}

extern "C" int orbfe_sim3_iterate(orbfe_sim3* h, int solver_index, int n_iterations, orbfe_sim3_state_t* state,
                                  orbfe_sim3_iterate_t* out) {
  if (!h || !state || !out || n_iterations < 0 || out->mask_words < 0 || state->iterations < 0)
    return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_iterate: bad argument");
  if (solver_index < 0 || solver_index >= (int)h->last.size())
    return orbfe_set_error(ORBFE_ERR_STATE, "orbfe_sim3_iterate: no such solver in the last solve");
  const Sim3Last& L = h->last[solver_index];
  if (out->inlier_mask && out->mask_words < (L.n + 63) / 64)
    return orbfe_set_error(ORBFE_ERR_CAPACITY, "orbfe_sim3_iterate: mask_words below ceil(n / 64)");
  out->accepted = -1;
  out->no_more = 0;
  out->n_inliers = 0;
  memset(out->t12, 0, sizeof(out->t12));
  if (out->inlier_mask) memset(out->inlier_mask, 0, 8 * (size_t)out->mask_words);
  if (L.n < L.min_inliers) {
    out->no_more = 1;
    return ORBFE_OK;
  }
  if (state->best >= L.n_eval) return orbfe_set_error(ORBFE_ERR_ARG, "orbfe_sim3_iterate: state is not this solver's");
  const int32_t* cnt = reinterpret_cast<const int32_t*>(h->res.h + L.o_cnt);
  int cur = 0;
  while (state->iterations < L.max_its && cur < n_iterations && state->iterations < L.n_eval) {
    cur++;
    const int k = state->iterations++;
    if (cnt[k] >= state->best_inliers) {
      state->best_inliers = cnt[k];
      state->best = k;
      if (cnt[k] > L.min_inliers) {
        out->accepted = k;
        out->n_inliers = cnt[k];
        memcpy(out->t12, h->res.h + L.o_t12 + 48 * (size_t)k, 48);
        if (out->inlier_mask) memcpy(out->inlier_mask, h->res.h + L.o_mask + 8 * (size_t)L.words * k, 8 * (size_t)L.words);
        return ORBFE_OK;
      }
    }
  }
  if (state->iterations >= L.max_its) out->no_more = 1;
  return ORBFE_OK;
}
